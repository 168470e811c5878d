"""Sorted order on resident columns (DeviceColumns.sort_order, fqsx_cols_sort_order): the read order of `-om s` computed where
the store keeps the reads -- several allocations, one per parsed chunk -- against the reference-equivalent host sort
(hostpipe.sorted_order_exact) and against the host-column path (codec.sort_order) on the same records; what the call holds on
the device; and compress_fastq(resident=True, order="s") / `e -resident -om s`, which no longer bring the base column to the
host.  Every comparison is exact.  Emulation build and, marked gpu, device 0."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import check_full_file_digest
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DeviceColumns, FqsxError, parse_fastq, sort_order
from fqsqueezer_amd.fqsfile import compress_fastq
from fqsqueezer_amd.synth import fastq_text, synth_c25_text
from test_device_columns import LENGTHS
from test_fqs_compress import MODES, WHERE, _lib, texts

COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 5600]   # around the 64 lanes of a wave and the 2048 reads of a sort tile
SHORT = [b"", b"A", b"AC", b"ACG", b"T", b"N", b"TTT"]   # fewer than four bases: a missing position is 3 in the bin, 0 in the key
VAR = "FQSX_TEST_ALLOC_FAIL"
E_ARG, E_NOMEM = -1, -4   # include/fqsx.h


# ---- reads --------------------------------------------------------------------------------------------------------------------------
def _odd_reads(n: int):
    """In the manner of test_sort._odd_records: N against T, other IUPAC and lower-case bytes (all code 3), proper prefixes, exact
    duplicates, reads equal under N->T, lengths 4..300.  The derived reads follow the reads they come from, chunks later."""
    rng = np.random.Generator(np.random.PCG64(77))
    alpha = np.frombuffer(b"ACGTACGTACGTACGTNNRYKMacgtn", dtype=np.uint8)
    seqs = []
    for i in range((n + 1) // 2):
        L = int(rng.integers(4, 60)) if i % 3 else int(rng.integers(60, 300))
        seqs.append(alpha[rng.integers(0, len(alpha), L)].tobytes())
    for i in range(n - len(seqs)):
        s = seqs[i]
        seqs.append(s if i % 3 == 0 else s[:max(4, len(s) // 2)] if i % 3 == 1 else s.replace(b"N", b"T"))
    return seqs


def _length_reads(n: int):
    """Read lengths through LENGTHS of test_device_columns in a seeded order, every fifth read one of SHORT in turn"""
    rng = np.random.default_rng(5)
    ln = np.array(LENGTHS)[rng.integers(0, len(LENGTHS), n)]
    seqs = [np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, k)].tobytes() for k in ln]
    for j, i in enumerate(range(0, n, 5)):
        seqs[i] = SHORT[j % len(SHORT)]
    return seqs


def _fixed_reads(n: int):
    """100 bp of A, C, G, T only, every seventh read a copy of an earlier one"""
    rng = np.random.default_rng(9)
    seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100)].tobytes() for _ in range(n)]
    for i in range(3, n, 7):
        seqs[i] = seqs[i // 3]
    return seqs


READS = {"odd": _odd_reads, "lengths": _length_reads, "fixed": _fixed_reads}


def _text_of(seqs) -> bytes:
    return fastq_text([b"@r%d" % i for i in range(len(seqs))], seqs, [b"I" * len(s) for s in seqs])


def _want_of(seqs):
    """the reference-equivalent host sort of the reads: one index array per non-empty bin"""
    return hp.sorted_order_exact(hp.Records([b"@r%d" % i for i in range(len(seqs))], list(seqs), [b"I" * len(s) for s in seqs]))


@functools.lru_cache(maxsize=None)
def _case(kind: str, n: int):
    """(reads, text, expected order): made once, shared by the emulation and the device case"""
    seqs = READS[kind](n)
    return seqs, _text_of(seqs), _want_of(seqs)


def _chunk_bytes(text: bytes, seqs, chunks: int = 6) -> int:
    """bytes of text per parsed chunk for about `chunks` chunks, never below the longest record (so that every parsed chunk
    holds a record and the parser's chunk count is the store's)"""
    return max(len(text) // chunks + 1, 2 * max(len(s) for s in seqs) + 32)


def _resident(text: bytes, lib, max_chunk_bytes: int = 0):
    st = {}
    return parse_fastq(text, lib_path=lib, max_chunk_bytes=max_chunk_bytes, stats=st, resident=True), st["chunks"]


def _assert_same_bins(got, want, what: str):
    assert len(got) == len(want), f"{len(got)} bins, {what} has {len(want)}"
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"non-empty bin #{b}: order differs from {what}"


# ---- 1. the order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", list(READS))
def test_order_of_a_store_of_several_chunks_equals_the_reference_and_the_host_columns(where, request, kind, n):
    lib = _lib(where, request)
    seqs, text, want = _case(kind, n)
    host = parse_fastq(text, lib_path=lib)
    dev, chunks = _resident(text, lib, _chunk_bytes(text, seqs))
    try:
        assert len(dev) == len(host) == n
        assert chunks >= 5 if n >= 63 else chunks == 1, chunks
        st = {}
        got = dev.sort_order(stats=st)
        _assert_same_bins(got, want, "hostpipe.sorted_order_exact")
        _assert_same_bins(got, sort_order(host.bases, host.read_off, lib_path=lib), "codec.sort_order on the host columns")
        assert sorted(np.concatenate(got).tolist()) == list(range(n))
        if kind == "fixed":
            assert st["passes"] == 25, st   # 100 / 4 passes over the N->T codes: no length pass, no raw-byte pass
    finally:
        dev.close()


@pytest.mark.parametrize("where", WHERE)
def test_order_of_a_store_of_one_chunk(where, request):
    lib = _lib(where, request)
    seqs, text, want = _case("odd", 2049)
    dev, chunks = _resident(text, lib)
    try:
        assert chunks == 1 and len(dev) == 2049
        _assert_same_bins(dev.sort_order(), want, "hostpipe.sorted_order_exact")
    finally:
        dev.close()


@pytest.mark.parametrize("where", WHERE)
def test_an_empty_store_has_no_bins(where, request):
    cols = DeviceColumns(lib_path=_lib(where, request))
    try:
        st, before = {}, cols.info()
        assert cols.sort_order(stats=st) == [] and st == {"passes": 0, "scratch_bytes": 0}
        assert cols.info() == before
    finally:
        cols.close()


def test_the_short_reads_go_to_the_bins_of_the_reference():
    """The expected orders above come from hostpipe.sorted_order_exact, so its bins are pinned here by hand: a position past the
    end of the read counts as 3 (application.cpp:383-391).  "A" is in bin 0333 = 63, not with "AAAAC" in bin 0; "ACG" shares
    bin 0123 = 27 with "ACGT", the shorter first; "", "N" and "TTT" are in bin 255 in the order of their N->T codes."""
    got = _want_of([b"AAAAC", b"A", b"", b"ACG", b"ACGT", b"TTT", b"N"])
    assert [g.tolist() for g in got] == [[0], [3, 4], [1], [2, 6, 5]]


# ---- 2. equal reads in different chunks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_equal_reads_in_different_chunks_keep_the_order_of_the_reference(where, request):
    """One read 40 times, every 15th record, among 560 others of its bin: std::sort leaves reads that compare equal in an order
    that depends on the order it met them in, so the replay on the host has to see the bin in record order."""
    lib = _lib(where, request)
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    same = b"ACGT" + acgt[rng.integers(0, 4, 46)].tobytes()
    seqs = [same if i % 15 == 0 else b"ACGT" + acgt[rng.integers(0, 4, int(rng.integers(0, 90)))].tobytes() for i in range(600)]
    text = _text_of(seqs)
    chunk = _chunk_bytes(text, seqs)
    assert chunk >= 15 * (2 * 94 + 16)   # 15 consecutive records fit a chunk several times over: the read is in every chunk
    dev, chunks = _resident(text, lib, chunk)
    try:
        assert chunks >= 5
        got, want = dev.sort_order(), _want_of(seqs)
        assert len(want) == 1 and seqs.count(same) == 40
        _assert_same_bins(got, want, "hostpipe.sorted_order_exact")
        at = np.flatnonzero(np.isin(got[0], np.arange(0, 600, 15)))
        assert len(at) == 40 and at[-1] - at[0] == 39   # (the equal reads are neighbours in the order)
    finally:
        dev.close()


# ---- 3. the column never reaches the host, and is never doubled ---------------------------------------------------------------------------
def _no_bases_to_host(self):
    raise AssertionError("the base column was brought to the host")


@pytest.mark.parametrize("where", WHERE)
def test_resident_sorted_compress_never_brings_the_bases_to_the_host(where, request, monkeypatch):
    lib, st = _lib(where, request), {}
    monkeypatch.setattr(DeviceColumns, "bases_to_host", _no_bases_to_host)
    data = compress_fastq(texts("c4"), resident=True, order="s", threads=4, genome_size_mbp=1, lib_path=lib, stats=st)
    records = st["columns"][0]["records"]
    assert records == 3000 and sum(b.n_reads for b in hp.parse_fqs(data)[1]) == records
    assert st["sort"]["resident"] is True and st["sort"]["passes"] > 0
    assert 0 < st["sort"]["scratch_bytes"] <= 32 * records + 4096, st["sort"]
    host = {}
    compress_fastq(texts("c4")[:20000].rsplit(b"\n@", 1)[0] + b"\n", order="s", threads=4, genome_size_mbp=1, lib_path=lib, stats=host)
    assert host["sort"]["resident"] is False and host["sort"]["batches"] == 1 and "scratch_bytes" not in host["sort"]


@pytest.mark.parametrize("where", WHERE)
def test_the_sort_holds_32_bytes_a_record_at_most_and_leaves_the_store_as_it_was(where, request):
    """per record 8 address + 4 length + 1 bin + 8 permutations + 4 flags + 4 rank bytes, about 0.5 for the tiles' histograms
    and info; the digit tables and a copy of the chunk table are within the 4096"""
    lib = _lib(where, request)
    seqs, text, want = _case("odd", 5600)
    dev, chunks = _resident(text, lib, _chunk_bytes(text, seqs))
    try:
        assert 5 <= chunks <= 16
        before, st = dev.info(), {}
        assert before["device_bytes_peak"] == before["device_bytes"]
        got = dev.sort_order(stats=st)
        after = dev.info()
        bound = 32 * 5600 + 4096
        assert 29 * 5600 <= st["scratch_bytes"] <= bound, st
        assert after["device_bytes_peak"] - before["device_bytes"] == st["scratch_bytes"]
        assert dict(after, device_bytes_peak=0) == dict(before, device_bytes_peak=0)
        _assert_same_bins(got, want, "hostpipe.sorted_order_exact")
        idx = np.arange(5600, dtype=np.int64)[::-1]   # and the store still cuts blocks
        assert np.array_equal(dev.download(dev.block_dev(idx).bases, int(dev.read_off[-1])), parse_fastq(text, lib_path=lib).block(idx)[0])
    finally:
        dev.close()


# ---- 4. the same file -----------------------------------------------------------------------------------------------------------------------
CHUNK = 200_000


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("name", ["c4", "c10"])
def test_single_end_resident_sorted_file_equals_the_host_column_file(where, request, name, qm, im):
    lib, st = _lib(where, request), {}
    kw = dict(threads=3, order="s", genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib)
    assert compress_fastq(texts(name), resident=True, max_chunk_bytes=CHUNK, stats=st, **kw) == compress_fastq(texts(name), **kw)
    assert st["parse"][0]["chunks"] >= 2 and st["sort"]["resident"] is True


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("name", ["c11", "c5"])
def test_paired_resident_sorted_file_equals_the_host_column_file(where, request, name, qm, im):
    lib, st = _lib(where, request), {}
    t1, t2 = texts(name)
    kw = dict(threads=2, order="s", genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib)
    assert compress_fastq(t1, t2, resident=True, max_chunk_bytes=CHUNK, stats=st, **kw) == compress_fastq(t1, t2, **kw)
    assert st["parse"][0]["chunks"] >= 2 and st["sort"]["resident"] is True   # (mate 1's store is sorted; the mates follow it)


@pytest.mark.parametrize("where", WHERE)
def test_resident_sorted_files_match_the_reference_digests(where, request, monkeypatch):
    lib = _lib(where, request)
    monkeypatch.setattr(DeviceColumns, "bases_to_host", _no_bases_to_host)
    kw = dict(order="s", genome_size_mbp=1, lib_path=lib, resident=True, max_chunk_bytes=CHUNK)
    check_full_file_digest(compress_fastq(texts("c10"), threads=2, quality_mode="lossless", id_mode="lossless", **kw), "c10_full_s_oo_t2.json")
    t1, t2 = texts("c11")
    check_full_file_digest(compress_fastq(t1, t2, threads=3, quality_mode="illumina_4", id_mode="lossless", **kw), "c11_pe_full_s_o4_t3.json")
    check_full_file_digest(compress_fastq(synth_c25_text(), threads=2, quality_mode="lossless", id_mode="lossless", **kw), "c25_plus_nolf_s_t2.json")


@pytest.mark.parametrize("where", WHERE)
def test_command_line_e_resident_om_s_writes_the_same_file(where, request, tmp_path, monkeypatch):
    from fqsqueezer_amd import fqsfile
    lib = _lib(where, request)
    monkeypatch.setattr(DeviceColumns, "bases_to_host", _no_bases_to_host)
    se = texts("c4")[:texts("c4").index(b"\n@rag.801\n") + 1]
    inp, out = tmp_path / "se.fq", tmp_path / "se.fqs"
    inp.write_bytes(se)
    args = ["e", "-s", "-om", "s", "-resident", "-t", "2", "-gs", "1", "-qm", "o", "-im", "o", "-out", str(out), str(inp)]
    assert fqsfile.main(args + (["-lib", lib] if lib else [])) == 0
    assert out.read_bytes() == compress_fastq(se, threads=2, order="s", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_every_allocation_of_the_sort_may_fail_and_the_call_be_repeated(where, request, monkeypatch):
    """FQSX_TEST_ALLOC_FAIL=k refuses the k-th allocation of a context, counted from its creation: a store has made one when it
    was created and one per chunk.  The sort makes twelve: chunk table, address, length, bin, two permutations, tile histograms,
    digit totals, digit offsets, flags, rank, tile info."""
    lib = _lib(where, request)
    monkeypatch.delenv(VAR, raising=False)
    seqs, text, want = _case("lengths", 2049)
    failed = []
    for j in range(-1, 32):
        dev, chunks = _resident(text, lib, _chunk_bytes(text, seqs))
        try:
            held = dev.info()["device_bytes"]
            monkeypatch.setenv(VAR, str(1 + chunks + j))
            try:
                got = dev.sort_order()
            except FqsxError as e:
                assert e.code == E_NOMEM and VAR in str(e), e
                assert dev.info()["device_bytes"] == held
                failed.append(j)
                monkeypatch.delenv(VAR)
                got = dev.sort_order()   # the same call again, on the same store
            finally:
                monkeypatch.delenv(VAR, raising=False)
            assert dev.info()["device_bytes"] == held
            _assert_same_bins(got, want, "hostpipe.sorted_order_exact")
        finally:
            dev.close()
        if j >= 0 and j not in failed:
            break
    assert failed == list(range(12)), failed   # (j = -1, the last chunk's allocation, is behind the store already)


@pytest.mark.parametrize("where", WHERE)
def test_null_outputs_are_refused(where, request):
    from fqsqueezer_amd.codec import load_library
    lib = load_library(_lib(where, request))
    dev, _ = _resident(_case("fixed", 65)[1], _lib(where, request))
    try:
        order, bins = np.zeros(65, dtype=np.uint32), np.full(257, 7, dtype=np.uint32)
        assert lib.fqsx_cols_sort_order(dev._h, None, bins.ctypes.data, None) == E_ARG
        assert lib.fqsx_cols_sort_order(dev._h, order.ctypes.data, None, None) == E_ARG
        assert lib.fqsx_cols_sort_order(None, order.ctypes.data, bins.ctypes.data, None) == E_ARG
        assert (bins == 7).all() and not order.any()
        info = (C.c_uint64 * 4)()
        assert lib.fqsx_cols_sort_order(dev._h, order.ctypes.data, bins.ctypes.data, info) == 0
        assert bins[0] == 0 and bins[256] == 65 and list(info)[2:] == [65, 0] and info[0] == 25
        _assert_same_bins([order[bins[b]:bins[b + 1]].astype(np.int64) for b in range(256) if bins[b + 1] > bins[b]], _case("fixed", 65)[2],
                          "hostpipe.sorted_order_exact")
    finally:
        dev.close()
