"""The GPU FASTQ parser (codec.parse_fastq -> hostpipe.Columns) against a pure-Python splitter that is the specification:
lines end at 0x0A only, four line feeds make a record, what follows the last fourth line feed is no record, any field may
be empty.  (Not hostpipe.read_fastq, which keeps a record that lacks its final line feed.)  Emulation build and, marked gpu,
device 0."""
import functools

import numpy as np
import pytest

from conftest import EMU_LIB, c4_records, c7_records, c20_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import parse_fastq
from fqsqueezer_amd.synth import fastq_text

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
TILE = 16384   # csrc/fqsx_fastq.h: FQSX_FQ_TILE


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


def check(text: bytes, lib, **kw):
    st = {}
    c = parse_fastq(text, device=0, lib_path=lib, stats=st, **kw)
    ids, id_off, bases, read_off, quals, plus_len, consumed, qual_off = split(text)
    assert len(c) == len(read_off) - 1
    assert st["consumed"] == consumed and st["tail_bytes"] == len(text) - consumed
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
@pytest.mark.parametrize("name", ["c4", "c7", "c20", "plus_ids", "crlf", "empty_fields"])
def test_columns_equal_the_specification(where, request, name):
    c, _ = check(texts(name), _lib(where, request))
    assert len(c) > 0 and (name != "plus_ids" or c.plus_len is not None)


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
@pytest.mark.parametrize("text", [b"", b"no line feed at all", b"\n", b"\n\n\n", b"\n\n\n\n", b"\n" * 5, b"\n" * 4099], ids=lambda t: "%dB" % len(t))
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
