"""The resident id column (codec.DeviceColumns.keep_ids, fqsx_cols_gather_ids / fqsx_cols_id_survey, fqsx_idg_encode_block_dev):
id lines cut on the device against the host gathers of hostpipe.Columns on the same text, the refusals (which leave the previous
block's ids alone), the survey against the pre-scan of the host id column, the id kernel fed from device memory against the same
kernel fed from host arrays, and compress_fastq(..., resident=True, resident_ids=True) / `e -resident-ids` against the host-column
path, the reference's own files and the host id coder's files.  Every comparison is byte for byte.  Emulation build and, marked
gpu, device 0; what the kernel answers with a change-over to the host coder runs on the emulation build only."""
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, check_full_file_digest
from fqsqueezer_amd import fqsfile
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DeviceColumns, FastqParser, FqsxError, IdCodec, parse_fastq
from fqsqueezer_amd.fqsfile import compress_fastq, compress_records
from fqsqueezer_amd.synth import fastq_text, synth_c25_text, synth_quals, synth_reads
from test_device_columns import BLOCKS, PATTERNS, _idx
from test_fqs_compress import MODES, WHERE, _lib, texts
from test_id_gpu import CASES, _arrays, _ids
from test_id_limits import PROBES, TABLE

LINES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024]   # bytes of an id line with its line feed: around the 16-byte groups of the copy
N_RECORDS = 5600                                              # (test_device_columns._idx draws from as many)
CHUNK = 200_000                                               # bytes of text per parsed chunk: the stores below hold 5 and more chunks
ALPHABET = np.frombuffer(b"abcdefgXYZ0123456789" * 3 + b"_/-|.: \0", dtype=np.uint8)   # mostly literals; separators, name ends, a NUL


def _same(a, b) -> bool:
    return a.dtype == b.dtype and np.array_equal(a, b)


def _edge_ids(seed: int, shift: int):
    rng = np.random.default_rng(seed)
    ln = np.array(LINES)[(rng.integers(0, len(LINES), N_RECORDS) + shift * np.arange(N_RECORDS)) % len(LINES)]
    ln[:len(LINES)] = LINES
    return [(b"@" + ALPHABET[rng.integers(0, len(ALPHABET), k - 2)].tobytes()) if k >= 2 else b"" for k in ln]


def _edge_text(seed: int, shift: int) -> bytes:
    """N_RECORDS records whose id lines run through LINES in a seeded order, so that the lines of a block start at every residue
    mod 16 in the column and in the block; shift: another order of lengths for the mate file.  Short reads of several lengths."""
    ids = _edge_ids(seed, shift)
    seqs = [b"ACGTN"[:1 + i % 5] * (1 + i % 7) for i in range(N_RECORDS)]
    return fastq_text(ids, seqs, [b"I" * len(s) for s in seqs])


@pytest.fixture(scope="module")
def parsed_columns():
    cache = {}
    yield cache
    for _, _, d1, d2 in cache.values():
        d1.close()
        d2.close()


def parsed(where, request):
    """(host Columns of mate 1, of mate 2, DeviceColumns that keep ids of mate 1, of mate 2) of the two edge texts, once per library"""
    cache = request.getfixturevalue("parsed_columns")
    if where not in cache:
        lib = _lib(where, request)
        t1, t2 = _edge_text(1, 0), _edge_text(2, 5)
        host = [parse_fastq(t, lib_path=lib) for t in (t1, t2)]
        stats = [{}, {}]
        dev = [parse_fastq(t, lib_path=lib, max_chunk_bytes=CHUNK, stats=st, resident=True, resident_ids=True) for t, st in zip((t1, t2), stats)]
        cache[where] = (host[0], host[1], dev[0], dev[1])
        assert all(st["chunks"] >= 5 for st in stats) and len(host[0]) == len(dev[0]) == N_RECORDS
        assert not np.array_equal(np.diff(host[0].id_off.view(np.int64)), np.diff(host[1].id_off.view(np.int64)))   # mates differ in length
        for h, d in zip(host, dev):
            assert len(d.ids) == 0 and _same(d.id_off, h.id_off) and _same(d.read_off, h.read_off)
            assert d.info()["id_bytes"] == len(h.ids) and d.keeps_ids
    return cache[where]


def _download(cols: DeviceColumns, blk):
    return cols.download(blk.ids, int(blk.off[-1])), cols.download(blk.d_off, 8 * len(blk.off)).view(np.uint64)


# ---- 1. the gather against the host columns -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", BLOCKS)
def test_ids_dev_equals_the_host_gather(where, request, n, pattern):
    h1, _, d1, _ = parsed(where, request)
    idx = _idx(pattern, n)
    want, want_off = h1.ids_of(idx)
    blk = d1.ids_dev(idx)
    ids, off = _download(d1, blk)
    assert _same(blk.off, want_off) and _same(off, want_off) and _same(ids, want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", BLOCKS)
def test_ids_pe_dev_equals_the_host_gather(where, request, n, pattern):
    h1, h2, d1, d2 = parsed(where, request)
    idx = _idx(pattern, n)
    want, want_off = h1.ids_of_pe(h2, idx)
    blk = d1.ids_pe_dev(d2, idx)
    ids, off = _download(d1, blk)
    assert len(blk.off) == 2 * n + 1 and _same(blk.off, want_off) and _same(off, want_off) and _same(ids, want)


@pytest.mark.parametrize("where", WHERE)
def test_a_smaller_id_block_after_a_larger_one_and_ids_of_on_the_store(where, request):
    h1, h2, d1, d2 = parsed(where, request)
    for n in (257, 63):
        idx = _idx("permutation", n)
        assert _same(_download(d1, d1.ids_dev(idx))[0], h1.ids_of(idx)[0])
        assert all(_same(a, b) for a, b in zip(d1.ids_of(idx), h1.ids_of(idx)))   # (the block downloaded: what the host id coder gets)
    for n in (256, 17):
        idx = _idx("reversed", n)
        assert _same(_download(d1, d1.ids_pe_dev(d2, idx))[0], h1.ids_of_pe(h2, idx)[0])
        assert all(_same(a, b) for a, b in zip(d1.ids_of_pe(d2, idx), h1.ids_of_pe(h2, idx)))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ids_first", [False, True], ids=["bases_then_ids", "ids_then_bases"])
def test_a_blocks_bases_and_its_ids_are_valid_together(where, request, ids_first):
    h1, h2, d1, d2 = parsed(where, request)
    idx = _idx("permutation", 300)
    if ids_first:
        iblk, blk = d1.ids_pe_dev(d2, idx), d1.block_pe_dev(d2, idx)
    else:
        blk, iblk = d1.block_pe_dev(d2, idx), d1.ids_pe_dev(d2, idx)
    n = int(blk.off[-1])
    assert _same(d1.download(blk.bases, n), h1.block_pe(h2, idx)[0]) and _same(d1.download(blk.quals, n), h1.quals_of_pe(h2, idx)[0])
    assert _same(d1.download(blk.d_off, 8 * len(blk.off)).view(np.uint64), blk.off)
    ids, off = _download(d1, iblk)
    assert _same(ids, h1.ids_of_pe(h2, idx)[0]) and _same(off, iblk.off)


# ---- 2. refusals: the id buffers keep the previous block --------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_bad_index_or_length_is_refused_and_the_previous_ids_stay(where, request, paired):
    _, _, d1, d2 = parsed(where, request)
    mate = d2 if paired else None
    good = _idx("permutation", 300)
    blk = d1.ids_pe_dev(d2, good) if paired else d1.ids_dev(good)
    before = [x.copy() for x in _download(d1, blk)]
    unchanged = lambda: all(_same(a, b) for a, b in zip(before, _download(d1, blk)))   # noqa: E731
    bad_idx = good.copy()
    bad_idx[170] = N_RECORDS                 # one past the last record
    with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1"):
        d1.gather_ids(bad_idx, blk.off, mate)
    assert unchanged()
    for delta in (1, -1):                    # one line a byte longer / shorter than the store holds (its neighbour the other way)
        bad_off = blk.off.copy()
        k = 40
        bad_off[k] = bad_off[k] + np.uint64(1) if delta > 0 else bad_off[k] - np.uint64(1)
        with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1"):
            d1.gather_ids(good, bad_off, mate)
        assert unchanged()
    longer = blk.off.copy()
    longer[-1] += np.uint64(1)               # the last line: its destination would also end past the block
    with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1"):
        d1.gather_ids(good, longer, mate)
    assert unchanged()
    again = _download(d1, d1.gather_ids(good, blk.off, mate))   # and the store still cuts the block
    assert all(_same(a, b) for a, b in zip(before, again))


@pytest.mark.parametrize("where", WHERE)
def test_a_store_or_a_mate_without_ids_and_keep_ids_after_the_first_chunk_are_refused(where, request):
    lib = _lib(where, request)
    text = np.frombuffer(b"@a.1\nACGTA\n+\n!!!!!\n@b\n\n+\n\n@c:2 x\nGG\n+\n##\n", dtype=np.uint8)
    p, plain, kept = FastqParser(lib_path=lib), DeviceColumns(lib_path=lib), DeviceColumns(lib_path=lib)
    try:
        kept.keep_ids()
        for cols in (plain, kept):
            cols.set_host_columns([p.columns_into(p.index(text), cols)])
        assert len(kept.ids) == 0 and plain.ids.tobytes() == b"@a.1\n@b\n@c:2 x\n" and _same(kept.id_off, plain.id_off)
        assert plain.info()["id_bytes"] == 0 and kept.info()["id_bytes"] == 15
        assert plain.id_survey() == {"keeps_ids": False, "id_bytes": 0, "max_line": 0, "max_tokens": 0, "max_name": 0, "max_name_tokens": 0}
        idx = np.array([2, 0, 1, 2])
        blk = kept.ids_dev(idx)
        assert _download(kept, blk)[0].tobytes() == b"@c:2 x\n@a.1\n@b\n@c:2 x\n"
        assert _download(kept, kept.ids_pe_dev(kept, idx[:2]))[0].tobytes() == b"@c:2 x\n@c:2 x\n@a.1\n@a.1\n"
        info = kept.info()
        with pytest.raises(FqsxError, match="fqsx_cols_keep_ids: -1"):
            plain.keep_ids()
        with pytest.raises(FqsxError, match="fqsx_cols_keep_ids: -1"):
            kept.keep_ids()
        assert kept.info() == info and not plain.keeps_ids
        off = np.zeros(len(idx) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.diff(plain.id_off.view(np.int64))[idx])
        with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1: .*keep ids"):
            plain.gather_ids(idx, off)
        off2 = np.zeros(2 * len(idx) + 1, dtype=np.uint64)
        off2[1:] = np.cumsum(np.repeat(np.diff(plain.id_off.view(np.int64))[idx], 2))
        with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1: .*keep ids"):
            kept.gather_ids(idx, off2, plain)
        assert _download(kept, kept.gather_ids(idx, off2, kept))[0].tobytes() == b"@c:2 x\n@c:2 x\n@a.1\n@a.1\n@b\n@b\n@c:2 x\n@c:2 x\n"
    finally:
        p.close()
        plain.close()
        kept.close()
    with pytest.raises(ValueError, match="resident_ids"):
        parse_fastq(text.tobytes(), lib_path=lib, resident_ids=True)
    with pytest.raises(ValueError, match="resident_ids"):
        compress_fastq(text.tobytes(), threads=2, order="o", genome_size_mbp=1, lib_path=lib, resident_ids=True)


@pytest.mark.parametrize("where", WHERE)
def test_an_empty_store_refuses_every_id_index(where, request):
    cols = DeviceColumns(lib_path=_lib(where, request))
    try:
        cols.keep_ids()
        assert cols.info()["records"] == 0 and cols.info()["id_bytes"] == 0
        assert cols.id_survey() == {"keeps_ids": True, "id_bytes": 0, "max_line": 0, "max_tokens": 0, "max_name": 0, "max_name_tokens": 0}
        blk = cols.ids_dev(np.zeros(0, dtype=np.int64))   # the empty block: a buffer of 64 spare bytes
        assert blk.ids and blk.d_off and _same(cols.download(blk.d_off, 8).view(np.uint64), np.zeros(1, dtype=np.uint64))
        before = cols.download(blk.ids, 64)
        with pytest.raises(FqsxError, match="fqsx_cols_gather_ids: -1"):
            cols.gather_ids(np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.uint64))
        assert _same(before, cols.download(blk.ids, 64))
    finally:
        cols.close()


# ---- 3. the survey ------------------------------------------------------------------------------------------------------------------------
def _verdict(sv: dict, id_mode: str) -> bool:
    return fqsfile._id_maxima_fit(id_mode, sv["max_line"], sv["max_tokens"], sv["max_name"], sv["max_name_tokens"])


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("what,probe", [pytest.param(p[1], p[2], id=("%s-%s" % p[:2]).replace(" ", "_")) for p in PROBES])
def test_the_surveys_verdict_is_the_prescans(where, request, what, probe):
    ordinary = [b"@ord.%d x:%d" % (i, 7 * i) for i in range(6)]
    ids = ordinary[:3] + [probe] + ordinary[3:]
    a, off = _arrays(ids)
    cols = parse_fastq(fastq_text(ids, [b"ACGT"] * len(ids), [b"IIII"] * len(ids)), lib_path=_lib(where, request), resident=True, resident_ids=True)
    try:
        sv = cols.id_survey()
        assert sv["keeps_ids"] and sv["id_bytes"] == len(a) and _same(cols.id_off, off)
        for id_mode in ("lossless", "instrument"):
            assert _verdict(sv, id_mode) is fqsfile._id_lines_fit_the_kernel(a, off, id_mode), (id_mode, sv)
        assert (sv["max_line"], sv["max_tokens"], sv["max_name"], sv["max_name_tokens"]) == _maxima([x + b"\n" for x in ids])
    finally:
        cols.close()


def _maxima(lines):
    """the four quantities of the survey, line by line"""
    lit = set(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz@")
    line = tokens = name = name_tokens = 0
    for x in lines:
        line, tokens = max(line, len(x)), max(tokens, sum(c not in lit for c in x))
        end = next((i for i, c in enumerate(x) if c in b". :"), None)
        if end is not None:
            name = max(name, len(x[:end].split(b"\0")[0]))
            name_tokens = max(name_tokens, sum(c not in lit for c in x[:end]) + 1)
    return line, tokens, name, name_tokens


@pytest.mark.parametrize("where", WHERE)
def test_the_surveys_maxima_on_the_edge_text(where, request):
    _, _, d1, d2 = parsed(where, request)
    for cols, (seed, shift) in ((d1, (1, 0)), (d2, (2, 5))):
        sv = cols.id_survey()
        want = _maxima([x + b"\n" for x in _edge_ids(seed, shift)])
        assert (sv["max_line"], sv["max_tokens"], sv["max_name"], sv["max_name_tokens"]) == want and want[0] == 1024 and min(want) > 0
        assert sv["id_bytes"] == int(cols.id_off[-1])


# ---- 4. the id kernel fed from device memory ------------------------------------------------------------------------------------------------
FAMILIES = sorted({c[1:] for c in CASES})


def _family_ids(kind: str, paired: bool, n: int):
    ids = _ids(kind, n, 5)
    if not paired:
        return [ids]
    return [[x + b"/1" for x in ids], [(x if i % 11 else x[:-1] + b"Z") + b"/2" for i, x in enumerate(ids)]]   # (test_id_gpu._compare's mates)


def _stores(mates, lib):
    return [parse_fastq(fastq_text(m, [b"ACGT"] * len(m), [b"IIII"] * len(m)), lib_path=lib, max_chunk_bytes=CHUNK, resident=True, resident_ids=True)
            for m in mates]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("id_mode,kind,paired", FAMILIES)
def test_encode_block_dev_equals_encode_block(where, request, id_mode, kind, paired, T):
    lib = _lib(where, request)
    sizes = [1, T - 1, T + 1, 3000]   # reads of the four blocks: workers without reads, ragged ranges
    if paired:
        sizes = [n // 2 for n in sizes]   # (pairs: even counts of reads)
    mates = _family_ids(kind, paired, sum(sizes))
    header = hp.make_header(T, "pe_original" if paired else "se_original", 1, id_mode=id_mode)
    stores = _stores(mates, lib)
    host, dev = IdCodec(header, lib_path=lib, device=0), IdCodec(header, lib_path=lib, device=0)
    try:
        at = 0
        for b, n in enumerate(sizes):
            idx = np.arange(at, at + n, dtype=np.int64)
            lines = [m[i] for i in range(at, at + n) for m in mates]
            at += n
            a, off = _arrays(lines)
            blk = stores[0].ids_pe_dev(stores[1], idx) if paired else stores[0].ids_dev(idx)
            assert _same(blk.off, off)
            want = host.encode_block(a, off, paired)
            assert dev.encode_block_dev(blk.ids, blk.d_off, blk.off, paired) == want, f"block {b}"
            assert dev.stats()["small_slots"] == host.stats()["small_slots"] and dev.stats()["big_slots"] == host.stats()["big_slots"], f"block {b}"
            assert np.array_equal(dev.state(), host.state()), f"block {b}"
        assert sum(len(s) for s in want) >= 8 * min(T, 3000)
    finally:
        host.close(); dev.close()
        for s in stores:
            s.close()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("what,bad,kind", [("a byte >= 128", b"@caf\xe9.2", 1), ("no instrument name", b"@abc/1", 2)])
def test_both_entry_points_refuse_an_id_alike(where, request, what, bad, kind):
    lib = _lib(where, request)
    ids = [b"@ok.1", bad, b"@ok.3", b"@ok.4"]
    header = hp.make_header(2, "se_original", 1, "none", "instrument")
    (store,) = _stores([ids], lib)
    host, dev = IdCodec(header, lib_path=lib, device=0), IdCodec(header, lib_path=lib, device=0)
    try:
        with pytest.raises(FqsxError, match=r"fqsx_idg_encode_block: -1: ") as e1:
            host.encode_block(*_arrays(ids))
        blk = store.ids_dev(np.arange(4))
        with pytest.raises(FqsxError, match=r"fqsx_idg_encode_block_dev: -1: ") as e2:
            dev.encode_block_dev(blk.ids, blk.d_off, blk.off)
        assert e1.value.code == e2.value.code == -1 and e1.value.staging is False and e2.value.staging is False
        assert host.error_kind() == dev.error_kind() == kind
        assert str(e1.value).split(": ", 2)[2] == str(e2.value).split(": ", 2)[2]
    finally:
        host.close(); dev.close(); store.close()


def test_the_host_id_coder_has_no_device_entry_point(built):
    with pytest.raises(FqsxError, match="encode_block_dev"):
        IdCodec(hp.make_header(2, "se_original", 1, "none", "lossless"), lib_path=EMU_LIB).encode_block_dev(0, 0, np.zeros(1, dtype=np.uint64))


# ---- 5. whole files -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("name", ["c4", "c10"])
def test_single_end_file_with_resident_ids_equals_the_host_column_file(where, request, name, order, qm, im):
    lib, st = _lib(where, request), {}
    kw = dict(threads=3, order=order, genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib)
    assert compress_fastq(texts(name), resident=True, resident_ids=True, max_chunk_bytes=CHUNK, stats=st, **kw) == compress_fastq(texts(name), **kw)
    host = parse_fastq(texts(name), lib_path=lib)
    assert st["ids_resident"] is True and st["gpu_ids"] is True and st["id_host_fallback"] is False
    assert st["parse"][0]["chunks"] >= 2 and st["columns"][0]["records"] == 3000 and st["columns"][0]["id_bytes"] == len(host.ids)
    if order == "o":   # (sorted order: the sort's scratch on the store is the peak)
        assert st["columns"][0]["device_bytes_peak"] == st["columns"][0]["device_bytes"]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("name", ["c11", "c5"])
def test_paired_file_with_resident_ids_equals_the_host_column_file(where, request, name, order, qm, im):
    lib, st = _lib(where, request), {}
    t1, t2 = texts(name)
    kw = dict(threads=3, order=order, genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib)
    assert compress_fastq(t1, t2, resident=True, resident_ids=True, max_chunk_bytes=CHUNK, stats=st, **kw) == compress_fastq(t1, t2, **kw)
    assert st["ids_resident"] is True and [c["id_bytes"] for c in st["columns"]] == [len(parse_fastq(t, lib_path=lib).ids) for t in (t1, t2)]


@pytest.mark.parametrize("where", WHERE)
def test_parsing_with_resident_ids_brings_no_id_byte_to_the_host_and_never_holds_the_file_twice(where, request):
    lib, st = _lib(where, request), {}
    host = parse_fastq(texts("c10"), lib_path=lib)
    cols = parse_fastq(texts("c10"), lib_path=lib, max_chunk_bytes=CHUNK, stats=st, resident=True, resident_ids=True)
    try:
        info = cols.info()
        assert len(cols.ids) == 0 and _same(cols.id_off, host.id_off) and np.array_equal(cols.record_sizes(), host.record_sizes())
        assert st["chunks"] >= 2 and info["id_bytes"] == len(host.ids) and info["bases"] == len(host.bases)
        assert info["device_bytes_peak"] == info["device_bytes"]   # one allocation per chunk that never moves, nothing freed meanwhile
        assert info["device_bytes"] <= 2 * info["bases"] + info["id_bytes"] + 16 * (len(host) + st["chunks"]) + 5 * 16 * st["chunks"] + 64
        cols.ids_dev(np.arange(len(host)))
        assert cols.info()["device_bytes_peak"] == cols.info()["device_bytes"]
    finally:
        cols.close()


@pytest.mark.parametrize("where", WHERE)
def test_files_with_resident_ids_are_the_reference_files(where, request):
    lib = _lib(where, request)
    kw = dict(genome_size_mbp=1, lib_path=lib, resident=True, resident_ids=True, max_chunk_bytes=CHUNK)
    data = compress_fastq(texts("c10"), threads=3, order="o", quality_mode="lossless", id_mode="lossless", **kw)
    assert data == open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()
    t1, t2 = texts("c11")
    check_full_file_digest(compress_fastq(t1, t2, threads=3, order="s", quality_mode="illumina_4", id_mode="lossless", **kw), "c11_pe_full_s_o4_t3.json")
    check_full_file_digest(compress_fastq(t1, t2, threads=2, order="o", quality_mode="lossless", id_mode="instrument", **kw), "c11_pe_full_o_io_t2.json")
    st = {}
    data = compress_fastq(synth_c25_text(), threads=3, order="o", quality_mode="lossless", id_mode="lossless", stats=st, **kw)
    assert data == open(os.path.join(GOLD, "c25_plus_nolf_o_t3.fqs"), "rb").read()
    assert st["parse"][0]["tail_bytes"] > 0 and st["columns"][0]["records"] == 1999 and st["ids_resident"] is True


# ---- 6. fall-backs to the host id coder (emulation only: nothing the kernel refuses is handed to a GPU) --------------------------------------
@pytest.mark.parametrize("id_mode,what,probe,fits", [pytest.param(*p, id=("%s-%s" % p[:2]).replace(" ", "_")) for p in TABLE])
def test_an_id_on_either_side_of_a_limit_compresses_to_the_host_coders_file(built, id_mode, what, probe, fits):
    ids = [b"@ord.%d x:%d" % (i, 7 * i) for i in range(80)]
    ids[61:61] = [probe, probe]
    rec = hp.Records(ids, synth_reads(len(ids), 60, 20000, 31), synth_quals(len(ids), 60, 31))
    want = compress_records(rec, 2, "o", 1, lib_path=EMU_LIB, id_mode=id_mode, gpu_ids=False)
    text = fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(len(rec))], [rec.qual_bytes(i) for i in range(len(rec))])
    st = {}
    assert compress_fastq(text, threads=2, order="o", genome_size_mbp=1, quality_mode="none", id_mode=id_mode, lib_path=EMU_LIB, stats=st,
                          resident=True, resident_ids=True) == want
    assert st["gpu_ids"] is fits and st["id_host_fallback"] is False and st["ids_resident"] is True


def test_the_4097th_name_changes_over_to_the_host_coder_in_mid_file(built):
    n = 5000
    ids = [b"@n%d.%d" % (i, i) for i in range(n)]
    rec = hp.Records(ids, synth_reads(n, 60, 20000, 32), synth_quals(n, 60, 32))
    want = compress_records(rec, 1, "s", 1, lib_path=EMU_LIB, id_mode="instrument", gpu_ids=False)
    text = fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(n)], [rec.qual_bytes(i) for i in range(n)])
    st = {}
    assert compress_fastq(text, threads=1, genome_size_mbp=1, quality_mode="none", lib_path=EMU_LIB, stats=st, resident=True, resident_ids=True) == want
    assert st["gpu_ids"] is True and st["id_host_fallback"] is True and st["ids_resident"] is True


# ---- 7. command line -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_command_line_e_resident_ids_then_d_round_trips(where, request, tmp_path):
    from fqsqueezer_amd import fqsread
    lib = _lib(where, request)
    extra = ["-lib", lib] if lib else []
    text = texts("c10")
    src, out, back = tmp_path / "in.fq", tmp_path / "out.fqs", tmp_path / "back.fq"
    src.write_bytes(text)
    assert fqsfile.main(["e", "-s", "-om", "o", "-resident-ids", "-t", "3", "-gs", "1", "-qm", "o", "-im", "o", "-out", str(out), str(src)] + extra) == 0
    assert out.read_bytes() == open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()
    assert fqsread.main(["d", str(out), "-out", str(back)] + extra) == 0
    assert back.read_bytes() == text
