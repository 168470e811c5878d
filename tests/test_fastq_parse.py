"""The GPU FASTQ parser (codec.parse_fastq -> hostpipe.Columns) against a pure-Python splitter that is the specification:
lines end at 0x0A only, four line feeds make a record, what follows the last fourth line feed is no record, any field may
be empty.  (Not hostpipe.read_fastq, which keeps a record that lacks its final line feed.)  Emulation build and, marked gpu,
device 0."""
import functools

import numpy as np
import pytest

from conftest import EMU_LIB, c4_records, c7_records, c20_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import FastqParser, parse_fastq
from fqsqueezer_amd.synth import fastq_text

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
TILE = 16384   # csrc/fqsx_fastq.h: FQSX_FQ_TILE
RTILE = 2048   # ... FQSX_FQ_RTILE
NAMES = ["c4", "c7", "c20", "plus_ids", "crlf", "empty_fields"]
EDGES = [b"", b"no line feed at all", b"\n", b"\n\n\n", b"\n\n\n\n", b"\n" * 5, b"\n" * 4099]
ROUND = 256    # tiles (record tiles) per round of k_fq_scan_tiles (k_fq_scan_rtiles) on the GPU: one per thread


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


def split(text: bytes):
    """(ids, id_off, bases, read_off, quals, plus_len, consumed): the specification"""
    ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    n = len(ends) // 4
    e = ends[:4 * n].reshape(n, 4)
    start = np.concatenate([[0], e[:-1, 3] + 1]) if n else np.zeros(0, dtype=np.int64)
    ids = b"".join(text[s:a + 1] for s, a in zip(start, e[:, 0]))
    bases = b"".join(text[a + 1:b] for a, b in zip(e[:, 0], e[:, 1]))
    quals = b"".join(text[c + 1:d] for c, d in zip(e[:, 2], e[:, 3]))
    off = lambda ln: np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    return (ids, off(e[:, 0] - start + 1), bases, off(e[:, 1] - e[:, 0] - 1), quals, e[:, 2] - e[:, 1] - 1,
            int(e[-1, 3]) + 1 if n else 0, off(e[:, 3] - e[:, 2] - 1))


def split_np(text: bytes):
    """split() without a Python loop, for texts of a million records: the same tuple, then the longest id line (with its line
    feed; 0 without a record) and whether any record's quality and base lengths differ.  The columns come from a mask over the
    text (the field of a byte is the number of line feeds before it, mod 4), the lengths from differences of the line ends."""
    t = np.frombuffer(text, dtype=np.uint8)
    lf = t == 10
    ends = np.flatnonzero(lf)
    n = len(ends) // 4
    e = ends[:4 * n].reshape(n, 4).astype(np.int64)
    consumed = int(e[-1, 3]) + 1 if n else 0
    t, lf = t[:consumed], lf[:consumed]
    field = (np.cumsum(lf, dtype=np.int64) - lf) & 3
    start = np.concatenate([[0], e[:-1, 3] + 1]) if n else np.zeros(0, dtype=np.int64)
    l_id, l_b, l_p, l_q = e[:, 0] - start + 1, e[:, 1] - e[:, 0] - 1, e[:, 2] - e[:, 1] - 1, e[:, 3] - e[:, 2] - 1
    off = lambda ln: np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    return (t[field == 0].tobytes(), off(l_id), t[(field == 1) & ~lf].tobytes(), off(l_b), t[(field == 3) & ~lf].tobytes(), l_p,
            consumed, off(l_q), int(l_id.max()) if n else 0, bool((l_q != l_b).any()))


def spec(text: bytes, big: bool = False):
    """split(), or split_np() for the large texts, with the two summary words in either case"""
    if big:
        return split_np(text)
    s = split(text)
    l_id, l_b, l_q = (np.diff(s[k].astype(np.int64)) for k in (1, 3, 7))
    return s + (int(l_id.max()) if len(l_id) else 0, bool((l_q != l_b).any()))


def check(text: bytes, lib, big: bool = False, **kw):
    st = {}
    c = parse_fastq(text, device=0, lib_path=lib, stats=st, **kw)
    ids, id_off, bases, read_off, quals, plus_len, consumed, qual_off, max_id_line, length_mismatch = spec(text, big)
    assert len(c) == len(read_off) - 1
    assert st["consumed"] == consumed and st["tail_bytes"] == len(text) - consumed
    assert st["max_id_line"] == max_id_line and st["length_mismatch"] is length_mismatch
    assert c.ids.tobytes() == ids and np.array_equal(c.id_off, id_off)
    assert c.bases.tobytes() == bases and np.array_equal(c.read_off, read_off)
    assert c.quals.tobytes() == quals and np.array_equal(c.qual_off, qual_off)
    assert (c.plus_len is None and bool((plus_len == 1).all())) or np.array_equal(c.plus_len, plus_len)
    return c, st


def _text(rec, **kw):
    return fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(len(rec))], [rec.qual_bytes(i) for i in range(len(rec))], **kw)


@functools.lru_cache(maxsize=None)
def texts(name: str) -> bytes:
    if name == "c4":
        return _text(c4_records())
    if name == "c7":
        return _text(c7_records())
    if name == "c20":   # 5000 bp: lines longer than a tile, tiles without any line feed
        r1, r2 = c20_records()
        return b"".join(_text(hp.Records(r.ids[:40], r.seq[:40], r.qual[:40])) for r in (r1, r2))
    if name == "plus_ids":
        return _text(c7_records(), plus_id_every=3)
    if name == "crlf":
        return texts("c7")[:60000].replace(b"\n", b"\r\n")
    if name == "empty_fields":
        return b"@\nAC\n+\n!!\n" + b"@e1\n\n+\n\n" + b"\n\n\n\n" + b"@\n\n+x\n\n" + texts("c7")[:texts("c7").index(b"\n@", 3000) + 1] + b"@last\n\n+\n\n"
    raise KeyError(name)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", NAMES)
def test_columns_equal_the_specification(where, request, name):
    c, _ = check(texts(name), _lib(where, request))
    assert len(c) > 0 and (name != "plus_ids" or c.plus_len is not None)


def test_the_numpy_specification_equals_the_splitter():
    """split_np() against split() on every small text: the large cases rest on split_np() alone"""
    for text in [texts(name) for name in NAMES] + EDGES + [MR_SHAPES[0] * 3 + b"".join(MR_SHAPES) + b"@partial\nAC"]:
        a, b = spec(text), spec(text, big=True)
        assert len(a) == len(b) == 10
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else (x == y and type(x) is type(y))


def _tail_cuts():
    t = texts("c4")
    e = [i for i in range(len(t) - 400, len(t)) if t[i] == 10][-5:]   # the line feed before the last record, then its four
    cuts = {"after_lf1": e[1] + 1, "after_lf2": e[2] + 1, "after_lf3": e[3] + 1, "no_final_lf": e[4]}
    for k in range(4):
        cuts["mid_line%d" % (k + 1)] = (e[k] + 2 + e[k + 1]) // 2   # (the one-byte separator line: between its `+` and its line feed)
    return t, e[0] + 1, cuts


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("cut", ["after_lf1", "after_lf2", "after_lf3", "mid_line1", "mid_line2", "mid_line3", "mid_line4", "no_final_lf"])
def test_a_partial_last_record_is_not_returned(where, request, cut):
    t, last_start, cuts = _tail_cuts()
    assert last_start < cuts[cut] < len(t)
    c, st = check(t[:cuts[cut]], _lib(where, request))
    assert len(c) == 2999 and st["consumed"] == last_start   # `consumed` points at the partial record's first byte


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("text", EDGES, ids=lambda t: "%dB" % len(t))
def test_edges(where, request, text):
    c, st = check(text, _lib(where, request))
    assert len(c) == text.count(b"\n") // 4


@pytest.mark.parametrize("where", WHERE)
def test_every_length_residue_and_the_tile_boundary(where, request):
    """Prefixes of one text: all 16 residues of the length mod 16 (the tail of the text is not a whole 16-byte load), and
    tile size - 1 / tile size / tile size + 1 with a line feed as the last byte of one tile and as the first byte of the next."""
    lib = _lib(where, request)
    c4 = texts("c4")
    head = c4[:c4.index(b"\n@", TILE - 400) + 1]
    pad = TILE - 1 - len(head)
    assert 2 < pad < 400
    text = head + b"@" + b"p" * (pad - 1) + b"\n\n+\n\n" + c4[len(head):len(head) + 40000]   # id line ends at TILE - 1, an empty base line at TILE
    assert text[TILE - 1] == 10 and text[TILE] == 10
    lengths = [TILE - 1, TILE, TILE + 1] + [200 + k for k in range(16)] + [TILE + 3000 + k for k in range(16)] + [2 * TILE + k for k in range(-1, 2)]
    assert {n % 16 for n in lengths} == set(range(16))
    for n in lengths:
        check(text[:n], lib)


@pytest.mark.parametrize("where", WHERE)
def test_chunk_size_does_not_change_the_columns(where, request):
    lib = _lib(where, request)
    text = texts("c4")
    (ref, st0), (a, st1), (b, st2) = check(text, lib), check(text, lib, max_chunk_bytes=1024), check(text, lib, max_chunk_bytes=TILE + 1)
    assert st0["chunks"] == 1 and st1["chunks"] > 1 and st2["chunks"] > 1
    for c in (a, b):
        for f in ("ids", "id_off", "bases", "read_off", "quals", "qual_off"):
            assert np.array_equal(getattr(c, f), getattr(ref, f)), f
        assert c.plus_len is None and ref.plus_len is None


@pytest.mark.parametrize("where", WHERE)
def test_a_record_longer_than_the_chunk_doubles_the_chunk(where, request):
    c, st = check(texts("c20"), _lib(where, request), max_chunk_bytes=1024)   # a record is 10 KB
    assert len(c) == 80 and st["chunks"] > 1


@pytest.mark.parametrize("where", WHERE)
def test_a_path_is_read_in_chunks(where, request, tmp_path):
    f = tmp_path / "x.fq"
    f.write_bytes(texts("plus_ids"))
    st = {}
    c = parse_fastq(str(f), device=0, lib_path=_lib(where, request), max_chunk_bytes=5000, stats=st)
    ref, _ = check(texts("plus_ids"), _lib(where, request))
    assert st["chunks"] > 1 and c.bases.tobytes() == ref.bases.tobytes() and c.ids.tobytes() == ref.ids.tobytes()
    assert np.array_equal(c.plus_len, ref.plus_len) and np.array_equal(c.record_sizes(), ref.record_sizes())


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b) == 2


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["c4", "plus_ids", "rect"])
def test_column_gathers_equal_the_record_functions(where, request, tmp_path, name):
    """Columns.block / ids_of / quals_of and the paired forms give what block_arrays / id_arrays / qual_arrays(_pe) give on
    read_fastq of the same text (ragged lists and the rectangular fast path), for random, repeated and empty index arrays."""
    lib = _lib(where, request)
    if name == "rect":
        r1, r2 = c20_records()
        t = [_text(hp.Records(r.ids[:30], r.seq[:30], r.qual[:30])) for r in (r1, r2)]
    else:
        lines = texts(name).split(b"\n")
        half = (len(lines) // 8) * 4
        t = [b"\n".join(lines[:half]) + b"\n", b"\n".join(lines[half:2 * half]) + b"\n"]
    recs, cols = [], []
    for m, x in enumerate(t):
        f = tmp_path / ("m%d.fq" % m)
        f.write_bytes(x)
        recs.append(hp.read_fastq(str(f)))
        cols.append(parse_fastq(x, device=0, lib_path=lib))
    n = len(recs[0])
    assert n == len(recs[1]) == len(cols[0]) == len(cols[1]) and n > 0
    rng = np.random.default_rng(5)
    for idx in (np.arange(n), np.zeros(0, dtype=np.int64), rng.integers(0, n, size=300), np.array([n - 1, 0, 0, n - 1, 7]), rng.permutation(n)[:n // 2]):
        idx = idx.astype(np.int64)
        for c, r in zip(cols, recs):
            assert _same(c.block(idx), hp.block_arrays(r, idx))
            assert _same(c.ids_of(idx), hp.id_arrays(r, idx))
            assert _same(c.quals_of(idx), hp.qual_arrays(r, idx))
        assert _same(cols[0].block_pe(cols[1], idx), hp.block_arrays_pe(recs[0], recs[1], idx))
        assert _same(cols[0].ids_of_pe(cols[1], idx), hp.id_arrays_pe(recs[0], recs[1], idx))
        assert _same(cols[0].quals_of_pe(cols[1], idx), hp.qual_arrays_pe(recs[0], recs[1], idx))
    for c, r in zip(cols, recs):
        assert np.array_equal(c.record_sizes(), r.record_sizes())


# ---- sizes at which the two single-workgroup scans carry from round to round ---------------------------------------------
# A round of k_fq_scan_tiles is ROUND tiles of text, a round of k_fq_scan_rtiles ROUND tiles of records: both texts below need
# three.  The specification of these texts is split_np().

@functools.lru_cache(maxsize=None)
def many_tiles() -> bytes:
    """c4 over and over, the repeats separated by records whose id lines all differ in length (no period in the tile size)"""
    c4, parts, size, k = texts("c4"), [], 0, 0
    while size <= 2 * ROUND * TILE + 1:
        sep = b"@" + b"s" * (1 + 37 * k % 301 + k) + b"\nACGT\n+\n!!!!\n"
        parts += [c4, sep]
        size += len(c4) + len(sep)
        k += 1
    return b"".join(parts)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("size", ["256t-1", "256t", "256t+1", "512t+1", "all"])
def test_the_tile_scan_carries_over_three_rounds(where, request, size):
    text = many_tiles()
    assert len(text) > 2 * ROUND * TILE + 1 and len({len(x) for x in text.split(texts("c4"))}) > len(text) // len(texts("c4"))
    n = {"256t-1": ROUND * TILE - 1, "256t": ROUND * TILE, "256t+1": ROUND * TILE + 1, "512t+1": 2 * ROUND * TILE + 1, "all": len(text)}[size]
    c, st = check(text[:n], _lib(where, request), big=True)
    assert st["chunks"] == 1 and len(c) > n // 400


MR_SHAPES = [b"\n\n\n\n", b"@a\nAC\n+\n!!\n", b"@bb\nACG\n+\n!!!\n", b"@\nA\n+x\n!\n"]
MR_N = 2 * ROUND * RTILE + 1500   # records: 513 record tiles, the last one partly filled


@functools.lru_cache(maxsize=None)
def many_records():
    """(text, start): MR_N tiny records drawn from MR_SHAPES; record i is text[start[i]:start[i + 1]]"""
    pick = np.random.default_rng(20).integers(0, len(MR_SHAPES), size=MR_N)
    start = np.concatenate([[0], np.cumsum(np.array([len(s) for s in MR_SHAPES])[pick])])
    text = b"".join([MR_SHAPES[k] for k in pick])
    assert len(text) == start[-1] and MR_N > 2 * ROUND * RTILE
    return text, start


def mr_variant(n_rec: int, at: int, record: bytes) -> bytes:
    """the first n_rec records of many_records() with record `at` replaced"""
    text, start = many_records()
    assert 0 <= at < n_rec <= MR_N
    return text[:start[at]] + record + text[start[at + 1]:start[n_rec]]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n_rec", [ROUND * RTILE, ROUND * RTILE + 1, MR_N], ids=["256rt", "256rt+1", "all"])
def test_the_record_tile_scan_carries_over_three_rounds(where, request, n_rec):
    text, start = many_records()
    c, st = check(text[:start[n_rec]], _lib(where, request), big=True)
    assert st["chunks"] == 1 and len(c) == n_rec and st["tail_bytes"] == 0
    assert n_rec < MR_N or (len(c) > 2 * ROUND * RTILE and 9 << 20 < len(text) < 11 << 20)
    rt = lambda off: np.diff(off[:len(c) // RTILE * RTILE + 1:RTILE].astype(np.int64))   # the record tiles' sums of one column
    assert all(len(np.unique(rt(off))) > 1 for off in (c.id_off, c.read_off, c.qual_off))
    assert (rt(c.id_off) != rt(c.read_off)).all()   # (and the quality lengths are the base lengths in this text)


# The one record that decides a summary word, at every place where the reduction changes hands: lanes 63 / 64 (two waves), 255 /
# 256 (a thread's first and second record of its tile), 2047 / 2048 (two record tiles), the last tile of the first round of
# k_fq_scan_rtiles and the first of its second (thread 0's second step of the strided reduction), a tile in the middle of the
# second round, and the last record of all.  The low places in a text of 5000 records, the others in as little as holds them.
LOW = 5000
PLACES = [(LOW, at) for at in (0, 63, 64, 255, 256, 2047, 2048)] + [
    (ROUND * RTILE + 1, ROUND * RTILE - 1), (ROUND * RTILE + 1, ROUND * RTILE), (MR_N, 300 * RTILE + 777), (MR_N, MR_N - 1)]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n_rec,at", PLACES, ids=["%d_of_%d" % (at, n) for n, at in PLACES])
def test_the_longest_id_line_is_found_wherever_it_is(where, request, n_rec, at):
    line = 8 if n_rec == LOW else 40 if n_rec < MR_N else 1100   # longer than every other (4 at most); the largest above the
    text = mr_variant(n_rec, at, b"@" + b"I" * (line - 2) + b"\nAC\n+\n!!\n")   # 1024 bytes the GPU id coder stages
    c, st = check(text, _lib(where, request), big=n_rec > LOW)
    assert st["max_id_line"] == line and not st["length_mismatch"] and st["chunks"] == 1
    assert int(np.diff(c.id_off.astype(np.int64)).argmax()) == at and len(c) == n_rec


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n_rec,at", PLACES, ids=["%d_of_%d" % (at, n) for n, at in PLACES])
def test_the_only_length_mismatch_is_found_wherever_it_is(where, request, n_rec, at):
    text = mr_variant(n_rec, at, b"@m\nAC\n+\n!!!\n")   # one quality byte more than bases
    c, st = check(text, _lib(where, request), big=n_rec > LOW)
    assert st["length_mismatch"] is True and st["max_id_line"] == 4 and st["chunks"] == 1 and len(c) == n_rec
    assert np.array_equal(c.qual_off[:at + 1], c.read_off[:at + 1]) and bool((c.qual_off[at + 1:] == c.read_off[at + 1:] + 1).all())


# ---- the two ranking paths of k_fq_index inside one tile -------------------------------------------------------------
def _mixed_tile(residue: int) -> bytes:
    """One tile whose four rounds of 4096 bytes (256 units of 16 bytes: one per thread, 64 per wave) are: at most one line feed per
    unit; the same but for one unit of the third wave with two; a line feed on the last byte of the first wave and one on the
    first byte of the second, then a run of units without any; sixteen per unit.  residue: the tile's line feeds mod 4."""
    t = np.full(TILE, ord("x"), dtype=np.uint8)
    unit = lambda rnd, u: 4096 * rnd + 16 * u
    for u in range(256):
        if u % 3 != 1:
            t[unit(0, u) + 7 * u % 16] = 10
        if u % 2 == 0:
            t[unit(1, u) + 5 * u % 16] = 10
        if u < 63 or u > 180:
            t[unit(2, u) + u % 16] = 10
    t[unit(1, 150) + 3] = 10   # (unit 150 of the second round, in the third wave, has one at byte 14 already)
    t[unit(2, 63) + 15] = t[unit(2, 64)] = 10
    t[unit(3, 0):] = 10
    for u in range(0, 256, 3):   # take line feeds out of the first round until the count fits
        if int((t == 10).sum()) % 4 == residue:
            break
        t[unit(0, u):unit(0, u + 1)] = ord("x")
    per_unit = (t.reshape(4, 256, 16) == 10).sum(axis=2)
    assert per_unit[0].max() == 1 and per_unit[2].max() == 1 and (per_unit[3] == 16).all() and (per_unit[2, 65:181] == 0).all()
    assert list(np.flatnonzero(per_unit[1] > 1)) == [150] and per_unit[1, 150] == 2 and t[unit(2, 63) + 15] == 10 == t[unit(2, 64)]
    assert int((t == 10).sum()) % 4 == residue
    return t.tobytes()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("residue", [1, 2, 3])
def test_ballot_and_scan_ranking_mixed_in_one_tile(where, request, residue):
    text = b"@" + b"l" * (TILE - 1) + _mixed_tile(residue) + b"r" * TILE + b"r" * 5   # no line feed in the tiles on either side
    c, st = check(text, _lib(where, request))
    assert len(c) == text.count(b"\n") // 4 > 1024 and st["tail_bytes"] > TILE and st["max_id_line"] > TILE


# ---- one handle, many chunks: the buffers (and the strides that follow their capacities) grow, stay and are reused ------
def _on_handle(p, text: bytes, big: bool = False):
    """index + columns of one chunk on the parser p, compared with the specification; -> (info, columns)"""
    ids, id_off, bases, read_off, quals, plus_len, consumed, qual_off, max_id_line, length_mismatch = spec(text, big)
    info = p.index(np.frombuffer(text, dtype=np.uint8))
    assert info == {"records": len(plus_len), "consumed": consumed, "id_bytes": len(ids), "bases": len(bases), "quals": len(quals),
                    "max_id_line": max_id_line, "length_mismatch": length_mismatch, "line_feeds": text.count(b"\n")}
    got = p.columns(info)
    for g, want in zip(got, (ids, id_off, bases, read_off, quals, qual_off, plus_len)):
        assert g.tobytes() == want if isinstance(want, bytes) else np.array_equal(g, want)
    return info, got


@pytest.mark.parametrize("where", WHERE)
def test_one_handle_large_small_larger_and_empty(where, request):
    p = FastqParser(0, _lib(where, request))
    try:
        _on_handle(p, texts("c4"))
        _on_handle(p, b"@a\nAC\n+\n!!\n")
        _on_handle(p, many_records()[0], big=True)
        _on_handle(p, texts("c20"))
        for none in (b"", b"abc"):
            info, got = _on_handle(p, none)
            assert info["records"] == 0 and [len(g) for g in got] == [0, 1, 0, 1, 0, 1, 0]
            assert all(int(got[k][0]) == 0 for k in (1, 3, 5))
        _on_handle(p, texts("c7"))
    finally:
        p.close()


@pytest.mark.parametrize("where", WHERE)
def test_columns_twice_and_index_twice(where, request):
    p = FastqParser(0, _lib(where, request))
    try:
        info, first = _on_handle(p, texts("plus_ids"))
        again = p.columns(info)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)) and len(again) == 7
        p.index(np.frombuffer(texts("c4"), dtype=np.uint8))   # indexed, its columns never asked for
        _on_handle(p, texts("empty_fields"))
        p.index(np.frombuffer(texts("c20"), dtype=np.uint8))
        info = p.index(np.zeros(0, dtype=np.uint8))
        assert info["records"] == 0 and [len(g) for g in p.columns(info)] == [0, 1, 0, 1, 0, 1, 0]
    finally:
        p.close()
