"""The GPU text assembler (codec.FastqText, csrc/fqsx_fqtext.h) against a pure-Python loop that is the specification: per
record id line + bases + "\\n+\\n" + qualities + "\\n", record i of a paired block to output i & 1.  On the small cases
fqsread.fastq_text / _take are held against that loop too; the large cases then rest on the numpy functions alone.
Emulation build and, marked gpu, device 0."""
import functools

import numpy as np
import pytest

from conftest import EMU_LIB, c20_records
from fqsqueezer_amd.codec import FastqText, FqsxError, parse_fastq
from fqsqueezer_amd.fqsread import _take, fastq_text
from test_fastq_parse import texts

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
RTILE = 2048   # csrc/fqsx_fqtext.h: FQSX_FT_RTILE
ROUND = 256    # record tiles per round of k_ft_scan_tiles on the GPU: one per thread
E_ARG = -1   # include/fqsx.h: FQSX_E_ARG


def test_the_copied_constants_are_the_kernels_own():
    """RTILE and ROUND decide whether case 3 crosses a round of the tile scan: read them where the kernels define them"""
    import os
    import re
    from conftest import ROOT
    src = {f: open(os.path.join(ROOT, "fqsqueezer_amd", "csrc", f)).read() for f in ("fqsx_fqtext.h", "fqsx_fastq.h", "fqsx_plat.h")}
    assert re.search(r"#define FQSX_FT_RTILE FQSX_FQ_RTILE\b", src["fqsx_fqtext.h"])
    assert int(re.search(r"#define FQSX_FQ_RTILE (\d+)u", src["fqsx_fastq.h"]).group(1)) == RTILE
    waves = int(re.search(r"#ifndef FQSX_EMU\n#define FQ_WAVES256 (\d+)u", src["fqsx_fastq.h"]).group(1))
    wave = int(re.search(r"#define FQ_WAVE (\d+)\n#define FQ_LANE \(\(u32\)\(threadIdx", src["fqsx_plat.h"]).group(1))
    assert re.search(r"for \(u32 b = 0; b < c\.n_tiles; b \+= FQ_N256\)", src["fqsx_fqtext.h"]) and waves * wave == ROUND
READ_LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151]
ID_LENS = [1, 2, 3, 17, 64, 65]
COUNTS = [0, 1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4097]


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


class Upload:
    """arrays into the memory the library under test calls device memory; keeps them alive"""

    def __init__(self, where):
        self.gpu, self.keep = where == "gpu", []

    def __call__(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        if a.size == 0:
            return 0
        if not self.gpu:
            self.keep.append(a)
            return a.ctypes.data
        import torch
        t = torch.from_numpy(a.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        self.keep.append(t)
        return t.data_ptr()


# ---- the specification ---------------------------------------------------------------------------------------------------
def spec(ids, seqs, quals, paired):
    out = ([], [])
    for i, (a, s, q) in enumerate(zip(ids, seqs, quals)):
        out[i & 1 if paired else 0].append(a + s + b"\n+\n" + q + b"\n")
    return b"".join(out[0]), b"".join(out[1])


def _off(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


def columns(ids, seqs, quals):
    """(ids, id_off, bases, read_off, quals) as the decoders give them"""
    a = lambda parts: np.frombuffer(b"".join(parts), dtype=np.uint8)   # noqa: E731
    return a(ids), _off([len(x) for x in ids]), a(seqs), _off([len(x) for x in seqs]), a(quals)


def numpy_text(ids, id_off, bases, read_off, quals, paired):
    """the same two outputs from fqsread.fastq_text / _take"""
    n = len(read_off) - 1
    text, rec_off = fastq_text(np.diff(read_off.astype(np.int64)).astype(np.uint32), bases, quals, ids, id_off)
    if not paired:
        return text.tobytes(), b""
    return tuple(_take(text, rec_off, np.arange(m, n, 2, dtype=np.int64)).tobytes() for m in (0, 1))


def assemble(t, up, ids, id_off, bases, read_off, quals, paired, how="dev", fill=0):
    """one block through FastqText: how = dev / host (where the ids are) / none (no ids); quals None: the fill byte"""
    kw = {}
    if how == "dev":
        kw = dict(ids=up(ids) or up(np.zeros(1, dtype=np.uint8)), id_len=up(np.diff(id_off.astype(np.int64)).astype(np.uint32)), id_bytes=len(ids))
    elif how == "host":
        kw = dict(ids=ids, id_len=np.diff(id_off.astype(np.int64)).astype(np.uint32))
    n = t.block(read_off, up(bases), up(quals) if quals is not None else None, paired=paired, qual_fill=fill, **kw)
    got = t.download(0).tobytes(), t.download(1).tobytes()
    assert n == (len(got[0]), len(got[1]))
    return got


def rand_records(n, seed, max_len=40, max_id=20):
    rng = np.random.default_rng(seed)
    L, il = rng.integers(0, max_len + 1, n), rng.integers(1, max_id + 1, n)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), k)) for k in L]
    quals = [bytes(rng.integers(33, 74, k, dtype=np.uint8)) for k in L]
    ids = [b"@" * min(1, k - 1) + bytes(rng.integers(48, 123, max(0, k - 2), dtype=np.uint8)) + b"\n" for k in il]
    return ids, seqs, quals


def check(where, request, ids, seqs, quals, paired, how="dev", small=True, t=None):
    cols = columns(ids, seqs, quals)
    want = numpy_text(*cols, paired)
    if small:
        assert want == spec(ids, seqs, quals, paired), "fqsread.fastq_text / _take differ from the specification"
    own = t is None
    t = t or FastqText(device=0, lib_path=_lib(where, request))
    try:
        got = assemble(t, Upload(where), *cols, paired, how)
    finally:
        if own:
            t.close()
    assert got[0] == want[0], "output 1"
    assert got[1] == want[1], "output 2"
    return want


# ---- 1. lengths and alignments -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alignment_records():
    combos = [(L, il) for L in READ_LENS for il in ID_LENS]
    rng = np.random.default_rng(16)
    ids, seqs, quals = [], [], []
    for rep in range(8):   # every combination eight times, rotated, so that the fields start everywhere
        for L, il in combos[5 * rep:] + combos[:5 * rep]:
            ids.append((b"@" + bytes(rng.integers(48, 123, 80, dtype=np.uint8)))[:il - 1] + b"\n")
            seqs.append(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L)))
            quals.append(bytes(rng.integers(33, 74, L, dtype=np.uint8)))
    return ids, seqs, quals


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_every_length_at_every_alignment(where, request, paired):
    ids, seqs, quals = alignment_records()
    assert {(len(s), len(i)) for s, i in zip(seqs, ids)} == {(L, il) for L in READ_LENS for il in ID_LENS}
    # where the base field and the quality field of every record start in its output, from the specification's sizes
    at, base_res, qual_res = [0, 0], set(), set()
    for k, (i, s) in enumerate(zip(ids, seqs)):
        m = k & 1 if paired else 0
        base_res.add((m, (at[m] + len(i)) % 16))
        qual_res.add((m, (at[m] + len(i) + len(s) + 3) % 16))
        at[m] += len(i) + 2 * len(s) + 4
    outs = (0, 1) if paired else (0,)
    assert base_res == {(m, r) for m in outs for r in range(16)} and qual_res == base_res, "the case does not cover every residue mod 16"
    check(where, request, ids, seqs, quals, paired)


# ---- 2. record counts at the lane, wave and tile edges -------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n", COUNTS)
def test_record_counts_single_end(where, request, n):
    check(where, request, *rand_records(n, 100 + n), False)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n", [n if n % 2 == 0 else n + 1 for n in COUNTS])
def test_record_counts_paired(where, request, n):
    check(where, request, *rand_records(n, 200 + n), True)


# ---- 3. more record tiles than one round of the tile scan holds ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_records():
    n = RTILE * ROUND + 1
    L = (np.arange(n) * 2654435761 >> 7) & 1
    bases = np.full(int(L.sum()), ord("G"), dtype=np.uint8)
    quals = (33 + np.arange(len(bases)) % 41).astype(np.uint8)
    ids = np.tile(np.frombuffer(b"@\n", dtype=np.uint8), n)
    cols = (ids, _off(np.full(n, 2)), bases, _off(L), quals)
    return cols, numpy_text(*cols, False)


@pytest.mark.parametrize("where", WHERE)
def test_one_record_more_than_a_round_of_the_tile_scan(where, request):
    cols, want = many_records()
    assert len(cols[3]) - 1 == RTILE * ROUND + 1 and 3_000_000 < len(want[0]) < 4_000_000
    t = FastqText(device=0, lib_path=_lib(where, request))
    try:
        got = assemble(t, Upload(where), *cols, False)
    finally:
        t.close()
    assert got[0] == want[0] and got[1] == b""


# ---- 4. pieces longer than anything staged -------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_reads_of_5000_bases(where, request, paired):
    r1, r2 = c20_records()
    if paired:
        recs = [(r, i) for i in range(20) for r in (r1, r2)]
    else:
        recs = [(r1, i) for i in range(40)]
    ids = [r.ids[i] + b"\n" for r, i in recs]
    seqs, quals = [r.seq_bytes(i) for r, i in recs], [r.qual_bytes(i) for r, i in recs]
    assert len(ids) == 40 and all(len(s) == 5000 for s in seqs)
    check(where, request, ids, seqs, quals, paired)


# ---- 5. constant ids, fill-byte qualities --------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("no_ids,no_quals", [(True, False), (False, True), (True, True)], ids=["no_ids", "no_quals", "neither"])
def test_constant_ids_and_fill_qualities(where, request, paired, no_ids, no_quals):
    ids, seqs, quals = rand_records(300, 5, max_len=70)
    fill = 33 + 7
    if no_ids:
        ids = [b"@\n"] * len(ids)
    if no_quals:
        quals = [bytes([fill]) * len(s) for s in seqs]
    want = spec(ids, seqs, quals, paired)
    c = columns(ids, seqs, quals)
    t = FastqText(device=0, lib_path=_lib(where, request))
    try:
        got = assemble(t, Upload(where), c[0], c[1], c[2], c[3], None if no_quals else c[4], paired, "none" if no_ids else "dev", fill)
    finally:
        t.close()
    assert got == want


# ---- 6. host ids and device ids ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_host_ids_give_the_bytes_device_ids_give(where, request, paired):
    recs = rand_records(2500, 6, max_id=90)
    a = check(where, request, *recs, paired, how="dev")
    b = check(where, request, *recs, paired, how="host")
    assert a == b


# ---- 7. a small block after a large one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_a_small_block_after_a_large_one(where, request):
    t = FastqText(device=0, lib_path=_lib(where, request))
    try:
        big = check(where, request, *rand_records(5000, 70, max_len=150), True, t=t)
        small = check(where, request, *rand_records(6, 71), True, t=t)
        assert t.text_bytes == (len(small[0]), len(small[1])) and len(small[0]) < len(big[0]) // 100
        single = check(where, request, *rand_records(3, 72), False, t=t)
        assert t.text_bytes == (len(single[0]), 0) and t.download(1).size == 0
    finally:
        t.close()


# ---- 8. refused calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("what", ["offsets_descend", "empty_id_line", "id_bytes_differ", "paired_odd"])
def test_a_refused_call_leaves_the_previous_text(where, request, what):
    up = Upload(where)
    t = FastqText(device=0, lib_path=_lib(where, request))
    try:
        first = rand_records(700, 80)
        before = assemble(t, up, *columns(*first), True)
        assert before == spec(*first, True)
        ids, id_off, bases, read_off, quals = columns(*rand_records(301, 81))
        id_len = np.diff(id_off.astype(np.int64)).astype(np.uint32)
        kw = dict(ids=up(ids), id_len=None, id_bytes=len(ids), paired=False)
        if what == "offsets_descend":
            read_off = read_off.copy()
            read_off[150] = read_off[149] - 1
            assert read_off[149] > 0 and read_off[-1] == len(bases)
        elif what == "empty_id_line":
            id_len[[7, 8]] = [0, id_len[7] + id_len[8]]   # (the sum stays what it was)
        elif what == "id_bytes_differ":
            longer = np.concatenate([ids, ids[:8]])   # (every line still lies inside the array)
            kw.update(ids=up(longer), id_bytes=len(longer))
        else:
            kw["paired"] = True
        kw["id_len"] = up(id_len)
        with pytest.raises(FqsxError) as e:
            t.block(read_off, up(bases), up(quals), **kw)
        assert e.value.code == E_ARG, str(e.value)
        assert t.text_bytes == (len(before[0]), len(before[1]))
        assert (t.download(0).tobytes(), t.download(1).tobytes()) == before, "the refused call touched the previous block's text"
        after = rand_records(64, 82)
        assert assemble(t, up, *columns(*after), False) == spec(*after, False)
    finally:
        t.close()


# ---- 9. the inverse of the parser ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["c4", "c7", "c20"])
def test_the_assembler_inverts_the_parser(where, request, name):
    lib = _lib(where, request)
    text = texts(name)
    c = parse_fastq(text, device=0, lib_path=lib)
    assert c.plus_len is None and np.array_equal(c.qual_off, c.read_off)   # `+` separators, complete records
    t = FastqText(device=0, lib_path=lib)
    try:
        got = assemble(t, Upload(where), c.ids, c.id_off, c.bases, c.read_off, c.quals, False)
    finally:
        t.close()
    assert got[0] == text and got[1] == b""
