"""The id coders at the id kernel's staging limits (csrc/fqsx_idk.h: a line of 1024 bytes with its line feed, 128 tokens, an
instrument name of 62 bytes, 4096 names per worker) and in their rare branches: move-to-front codes beyond 3, the mate comparison
over more than one round of 64 bytes, the exact edges of the numeric delta classes.  The reference's files of the c26 inputs
(tools/make_golden.py --only c26, synth.synth_c26) decide what is right: every block's id streams from the host coder and from
the kernel, the decoders' id lines and text, and the file the automatic choice between the two coders writes.  The pre-scan that
makes this choice (fqsfile._id_lines_fit_the_kernel) is held against the kernel id by id on both sides of every limit, and the
change-over to the host coder in mid-file against a file with more instrument names than the kernel's list holds.  Nothing the
kernel refuses is handed to a GPU: those cases run on the emulation build only.  Emulation build and, marked gpu, device 0."""
import functools
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, IM
from fqsqueezer_amd import fqsfile
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import FqsxError, IdCodec
from fqsqueezer_amd.fqsfile import compress_fastq, compress_records, compress_records_pe
from fqsqueezer_amd.fqsread import decompress_fastq, decompress_fastq_chunks
from fqsqueezer_amd.synth import C26, fastq_text, synth_c26, synth_quals, synth_reads
from test_id_decode import _tokens
from test_id_gpu import _arrays

INSIDE = [n for n in C26 if C26[n][5]]
OVER = [n for n in C26 if not C26[n][5]]
WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
CASES_INSIDE = [pytest.param("emu", n, id="emu-" + n) for n in INSIDE] + [pytest.param("gpu", n, id="gpu-" + n, marks=pytest.mark.gpu) for n in INSIDE]
CASES_ALL = CASES_INSIDE + [pytest.param("emu", n, id="emu-" + n) for n in OVER]   # (ids beyond the limits: emulation only)


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


@functools.lru_cache(maxsize=None)
def records(name):
    """the Records of a c26 input, one per mate file"""
    got = synth_c26(name)
    return tuple(hp.Records(got[2 * m], got[2 * m + 1], synth_quals(len(got[0]), 60, 26 + m)) for m in range(len(got) // 2))


@functools.lru_cache(maxsize=None)
def texts(name):
    return tuple(fastq_text(r.ids, [r.seq_bytes(i) for i in range(len(r))], [r.qual_bytes(i) for i in range(len(r))]) for r in records(name))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(the reference's file, the digests of what `fqs d` writes for it)"""
    tag = C26[name][0]
    return open(os.path.join(GOLD, tag + ".fqs"), "rb").read(), json.load(open(os.path.join(GOLD, tag + ".json")))


def _mode(name):
    tag, paired, om, im, T, inside = C26[name]
    return ("pe_" if paired else "se_") + ("sorted" if om == "s" else "original")


@functools.lru_cache(maxsize=None)
def block_lines(name):
    """the id lines (with their line feeds) of every container block, in the block's order (mates interleaved)"""
    recs = records(name)
    if len(recs) == 2:
        blks = hp.form_blocks_pe(recs[0], recs[1], _mode(name))
        return [[r.ids[int(i)] + b"\n" for i in idx for r in recs] for idx in blks]
    return [[recs[0].ids[int(i)] + b"\n" for i in idx] for idx in hp.form_blocks(recs[0], _mode(name), exact_ties=True)]


def _columns(lines):
    off = np.zeros(len(lines) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lines])
    return np.frombuffer(b"".join(lines), dtype=np.uint8), off


def _compress(name, lib, gpu_ids, stats=None):
    tag, paired, om, im, T, inside = C26[name]
    f = compress_records_pe if paired else compress_records
    return f(*records(name), T, om, 1, lib_path=lib, quality_mode="none", id_mode=IM[im], gpu_ids=gpu_ids, stats=stats)


# ---- conditions on the inputs: what the tests below can only show if the inputs hold it (checked from the inputs alone) -----------
def _name_of(line: bytes) -> bytes:
    name = line[:min(i for i, c in enumerate(line) if c in b". :")]
    return name.split(b"\0")[0]


def _mtf_classes(lines):
    """the classes of move-to-front codes (mtf.cpp:52-116, id.cpp:421-495) one worker meets on these lines"""
    lst, seen = [], set()
    for x in lines:
        name = _name_of(x)
        if name not in lst:
            seen.add("new")
        else:
            c = lst.index(name)
            lst.pop(c)
            seen.add("code 0" if c == 0 else "code 1" if c == 1 else ">= 256" if c >= 256 else "k = %d" % [k for k in range(7) if (2 << k) <= c < (4 << k)][0])
        lst.insert(0, name)
    return seen


MTF_CLASSES = {"new", "code 0", "code 1", ">= 256"} | {"k = %d" % k for k in range(7)}


def _workers(blocks, T):
    """the lines of every worker, block after block (a worker's models and its list of names last for the whole file)"""
    out = [[] for _ in range(T)]
    for lines in blocks:
        for w, (first, last) in enumerate(hp.partition_for_workers(len(lines), T)):
            out[w] += lines[first:last]
    return out


def test_c26_names_meet_every_class_of_move_to_front_code():
    blocks = block_lines("names")
    assert len({_name_of(x) for b in blocks for x in b}) == 300 and max(len(_name_of(x)) for b in blocks for x in b) == 62
    (one,) = _workers(blocks, 1)
    assert _mtf_classes(one) == MTF_CLASSES
    assert set().union(*[_mtf_classes(w) for w in _workers(blocks, 3)]) == MTF_CLASSES
    assert len(blocks) > 100   # (sorted order: a block per bin, so the lists are carried over many blocks)


# both edges of every size class of a numeric delta in idk_lossless / id_lossless (id.cpp:257-418); "+8" ends where ten digits end
DELTA_EDGES = {"small": (-1, 1), "one byte": (-123, -2, 2, 123), "+2 bytes": (124, 0xFFFF), "-2 bytes": (-124, -0xFFFF),
               "+3 bytes": (0x10000, 0xFFFFFF), "-3 bytes": (-0x10000, -0xFFFFFF), "+4 bytes": (0x1000000, 0xFFFFFFFF),
               "-4 bytes": (-0x1000000, -0xFFFFFFFF), "+8 bytes": (0x100000000, 9_999_999_999), "-8 bytes": (-0x100000000, -9_999_999_999)}


def _numeric_deltas(blocks, T):
    """per worker the deltas of the numeric tokens of consecutive lines with tokens of the same types (the first line of a block
    has no predecessor: ResetReadPrev)"""
    out = [set() for _ in range(T)]
    for lines in blocks:
        for w, (first, last) in enumerate(hp.partition_for_workers(len(lines), T)):
            prev = None
            for x in lines[first:last]:
                cur = _tokens(x)
                if prev is not None and len(cur) == len(prev) and all(a[:2] == b[:2] for a, b in zip(cur, prev)):
                    out[w] |= {int(a[2]) - int(b[2]) for a, b in zip(cur, prev) if a[0]}
                prev = cur
    return out


def test_c26_ids_limits_hold_every_edge_of_the_delta_classes_and_the_last_values_inside_the_limits():
    blocks = block_lines("ids_limits")
    for w, seen in enumerate(_numeric_deltas(blocks, 2)):
        for cls, edges in DELTA_EDGES.items():
            assert set(edges) <= seen, f"worker {w}: class {cls}: edges {set(edges) - seen} missing"
    for w, lines in enumerate(_workers(blocks, 2)):
        follows = lambda ok: any(ok(a) and ok(b) for a, b in zip(lines, lines[1:]))   # noqa: E731 -- twice in a row: plain, then same types
        assert follows(lambda x: len(x) == 1024), f"worker {w}: no two lines of 1024 bytes in a row"
        assert follows(lambda x: len(_tokens(x)) == 128 and not set(x) & set(b" :._/-|=#")), f"worker {w}: no two lines of 128 tokens in a row"
        assert follows(lambda x: x == b"@\n"), f"worker {w}"
        assert any([len(t[2]) for t in _tokens(x)][1:3] == [10, 11] and [t[0] for t in _tokens(x)][1:3] == [True, False] for x in lines), f"worker {w}"
        assert max(len(x) for x in lines) == 1024 and max(len(_tokens(x)) for x in lines) == 128


def test_c26_ids_over_adds_three_ids_beyond_the_limits_in_the_second_half():
    a, b = [x for blk in block_lines("ids_limits") for x in blk], [x for blk in block_lines("ids_over") for x in blk]
    added = [i for i, x in enumerate(b) if x not in a]
    assert len(b) == len(a) + 3 and [x for x in b if x in a] == a and min(added) >= len(b) // 2
    assert [len(b[i]) for i in added] == [1025, len(b[added[1]]), 1101] and len(_tokens(b[added[1]])) == 129
    assert not set(b[added[1]]) & set(b" :._/-|=#")


def test_c26_names_over_has_names_of_60_to_64_bytes():
    (lines,) = block_lines("names_over")
    assert len(lines) == 200 and {len(_name_of(x)) for x in lines} == {60, 61, 62, 63, 64}


def test_c26_pe_long_mates_differ_beyond_the_first_round_of_the_comparison():
    (lines,) = block_lines("pe_long")
    kinds = {"typical": 0, "in 64 .. na - 4": 0, "at na - 3": 0, "equal": 0, "lengths": 0}
    for a, b in zip(lines[0::2], lines[1::2]):
        assert 71 <= len(a) <= 201 and 71 <= len(b) <= 201
        d = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        if len(a) != len(b):
            kinds["lengths"] += 1
        elif a == b:
            kinds["equal"] += 1
        elif d == len(a) - 2:
            kinds["typical"] += a[-2:-1] == b"1" and b[-2:-1] == b"2"
        elif d == len(a) - 3:
            kinds["at na - 3"] += 1
        elif d >= 64:
            kinds["in 64 .. na - 4"] += 1
    assert kinds["in 64 .. na - 4"] + kinds["at na - 3"] >= 50 and min(kinds.values()) >= 50, kinds


# ---- the encoders against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,name", CASES_INSIDE)
def test_id_streams_of_both_coders_are_the_reference_files(where, request, name):
    lib = _lib(where, request)
    tag, paired, om, im, T, inside = C26[name]
    data, _ = fixture(name)
    header, ref_blocks = hp.parse_fqs(data)
    assert header == hp.make_header(T, _mode(name), 1, "none", IM[im])
    host, kern = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    blocks = block_lines(name)
    assert len(blocks) == len(ref_blocks)
    for g, (lines, ref) in enumerate(zip(blocks, ref_blocks)):
        assert len(lines) == ref.n_reads
        ids, off = _columns(lines)
        want = [ref.streams[w][hp.STREAM_ID] for w in range(T)]
        assert host.encode_block(ids, off, paired) == want, f"{tag}: block {g}: the host coder's id streams differ from the reference's"
        assert kern.encode_block(ids, off, paired) == want, f"{tag}: block {g}: the kernel's id streams differ from the reference's"
    host.close(); kern.close()
    assert _compress(name, lib, True) == data, f"{tag}: the file with the id kernel differs from the reference's"


@pytest.mark.parametrize("where", WHERE)
def test_every_move_to_front_class_in_one_worker_kernel_against_host_coder(where, request):
    """c26_names with T = 1, where one worker meets every class of code (the reference's file has T = 3): both directions"""
    lib = _lib(where, request)
    header = hp.make_header(1, "se_sorted", 1, "none", "instrument")
    enc_h, enc_k = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    dec_h, dec_k = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    for g, lines in enumerate(block_lines("names")):
        ids, off = _columns(lines)
        st = enc_h.encode_block(ids, off)
        assert enc_k.encode_block(ids, off) == st, f"block {g}"
        want = b"".join(_name_of(x) + b"\n" for x in lines)
        for dec in (dec_h, dec_k):
            got, _ = dec.decode_block(st, len(lines))
            assert got.tobytes() == want, f"block {g}"
    assert enc_k.state()[0, 2] == 300 and np.array_equal(enc_k.state(), dec_k.state())
    for c in (enc_h, enc_k, dec_h, dec_k):
        c.close()


# ---- the decoders against the reference --------------------------------------------------------------------------------------------
def _id_lines(text: bytes):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return lines[0:-1:4]


def _check_text(tag, d, mates):
    assert len(mates) == (2 if d["paired"] else 1)
    for m, t in enumerate(mates):
        ref = d["mate%d" % (m + 1)]
        ids = _id_lines(t)
        assert len(ids) == ref["reads"], f"{tag}: mate {m + 1}: number of reads"
        assert hashlib.sha256(b"".join(x + b"\n" for x in ids)).hexdigest() == ref["id_lines_sha256"], f"{tag}: mate {m + 1}: id lines differ from `fqs d`"
        assert len(t) == ref["fastq_bytes"] and hashlib.sha256(t).hexdigest() == ref["fastq_sha256"], f"{tag}: mate {m + 1}: text differs from `fqs d`"


@pytest.mark.parametrize("where,name", CASES_ALL)
def test_reference_files_decode_to_what_fqs_d_writes(where, request, name):
    lib = _lib(where, request)
    tag, paired, om, im, T, inside = C26[name]
    data, d = fixture(name)
    assert d["within_kernel_limits"] is inside
    for gpu_ids in (True, False):
        st = {}
        text = decompress_fastq(data, device=0, lib_path=lib, stats=st, gpu_ids=gpu_ids)
        _check_text(tag, d, text if paired else (text,))
        assert st["id_host_fallback"] is (gpu_ids and not inside), f"{tag}: 1024 bytes, 128 tokens and 62 bytes are inside the decoder's limits, what is beyond is not"
    st = {}
    chunks = list(decompress_fastq_chunks(data, device=0, lib_path=lib, stats=st))
    _check_text(tag, d, tuple(b"".join(c[m] for c in chunks) for m in (0, 1)) if paired else (b"".join(chunks),))
    assert st["id_host_fallback"] is (not inside)


# ---- the automatic choice ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,name", CASES_ALL)
def test_the_automatic_choice_writes_the_reference_file(where, request, name):
    lib = _lib(where, request)
    tag, paired, om, im, T, inside = C26[name]
    data, _ = fixture(name)
    st = {}
    assert _compress(name, lib, None, st) == data, f"{tag}: compress_records*"
    assert st["gpu_ids"] is inside and st["id_host_fallback"] is False
    t = texts(name)
    for resident in (False, True):
        st = {}
        got = compress_fastq(t[0], t[1] if paired else None, threads=T, order=om, genome_size_mbp=1, quality_mode="none", id_mode=IM[im], lib_path=lib,
                             stats=st, resident=resident)
        assert got == data, f"{tag}: compress_fastq, resident={resident}"
        assert st["gpu_ids"] is inside and st["id_host_fallback"] is False


# ---- pre-scan and kernel agree (the kernel side: emulation only) ----------------------------------------------------------------------
def _long(n, sep=b"."):
    return b"@nm" + sep + b"x" * (n - 4)


def _tokens_lossless(n_sep, sep):   # n_sep separators: n_sep + 1 tokens with the line feed
    return b"@a" + (sep + b"b") * n_sep


def _tokens_in_name(n_sep, sep):    # a name cut short by a NUL, n_sep separators before its '.': n_sep + 1 tokens with the terminator
    return b"@a\0" + sep * (n_sep - 1) + b".x"


# (id mode, what, the id, True: within the kernel's limits / False: beyond them / None: refused by both coders as a bad argument)
PROBES = [
    ("lossless", "line of 1024 bytes", _long(1023), True), ("lossless", "line of 1025 bytes", _long(1024), False),
    ("instrument", "line of 1024 bytes", _long(1023), True), ("instrument", "line of 1025 bytes", _long(1024), False),
    ("instrument", "line of 1024 bytes, name ends at ':'", _long(1023, b":"), True), ("instrument", "line of 1025 bytes, name ends at ' '", _long(1024, b" "), False),
    ("lossless", "128 tokens, ':'", _tokens_lossless(127, b":"), True), ("lossless", "129 tokens, ':'", _tokens_lossless(128, b":"), False),
    ("lossless", "128 tokens, ','", _tokens_lossless(127, b","), True), ("lossless", "129 tokens, ','", _tokens_lossless(128, b","), False),
    ("lossless", "128 tokens, tab", _tokens_lossless(127, b"\t"), True), ("lossless", "129 tokens, NUL", _tokens_lossless(128, b"\0"), False),
    ("instrument", "129 tokens, ':' (the name is the first)", _tokens_lossless(128, b":"), True),
    ("instrument", "300 tokens, ',', after the name", b"@a." + b",b" * 299, True),
    ("instrument", "128 tokens up to the name's end, '-'", _tokens_in_name(127, b"-"), True),
    ("instrument", "129 tokens up to the name's end, '-'", _tokens_in_name(128, b"-"), False),
    ("instrument", "128 tokens up to the name's end, ','", _tokens_in_name(127, b","), True),
    ("instrument", "129 tokens up to the name's end, ','", _tokens_in_name(128, b","), False),
    ("instrument", "name of 62 bytes", b"@" + b"n" * 61 + b".1", True), ("instrument", "name of 63 bytes", b"@" + b"n" * 62 + b".1", False),
    ("instrument", "name of 62 bytes, ':'", b"@" + b"n" * 61 + b":1", True), ("instrument", "name of 63 bytes, ' '", b"@" + b"n" * 62 + b" 1", False),
    ("instrument", "name of 200 bytes", b"@" + b"n" * 199 + b":1", False),
    ("lossless", "name of 63 bytes", b"@" + b"n" * 62 + b".1", True),
    ("lossless", "70 colons in 150 bytes", b"@" + b"ab:" * 9 + b":" * 61 + b"c" * 61, True),
    ("instrument", "70 colons in 150 bytes", b"@" + b"ab:" * 9 + b":" * 61 + b"c" * 61, True),
    ("instrument", "NUL after 3 bytes, name's end after 74", b"@ab\0" + b"c" * 70 + b".1", True),
    ("instrument", "NUL after 62 bytes", b"@" + b"c" * 61 + b"\0d.1", True), ("instrument", "NUL after 63 bytes", b"@" + b"c" * 62 + b"\0d.1", False),
    ("lossless", "NUL in the id", b"@ab\0" + b"c" * 70 + b".1", True),
    ("instrument", "no '.', ' ' or ':'", b"@abc/1", None), ("lossless", "no '.', ' ' or ':'", b"@abc/1", True),
    ("instrument", "no '.', ' ' or ':' in 1023 bytes", b"@" + b"c" * 1022, None),
    ("instrument", "bytes >= 128 after the name", b"@ok.1 caf\xe9 \xff", True),
]


def _prescan(ids, id_mode):
    """the verdict of both variants of the pre-scan"""
    a, off = _arrays(ids)
    listed = fqsfile._ids_fit_the_kernel(id_mode, hp.Records(ids, [], []))
    columns = fqsfile._id_columns_fit_the_kernel(SimpleNamespace(ids=a, id_off=off), int(np.diff(off.astype(np.int64)).max()), id_mode)
    assert listed == columns, "the list variant and the column variant of the pre-scan disagree"
    return listed


@pytest.mark.parametrize("id_mode,what,probe,fits", [pytest.param(*p, id=("%s-%s" % p[:2]).replace(" ", "_")) for p in PROBES])
def test_prescan_and_kernel_agree(built, id_mode, what, probe, fits):
    assert len(probe) == 150 or "150 bytes" not in what
    ordinary = [b"@ord.%d x:%d" % (i, 7 * i) for i in range(6)]
    ids = ordinary[:3] + [probe] * (1 if fits is False else 2) + ordinary[3:]   # (what fits: twice, for the path of equal token types too)
    assert _prescan(ordinary, id_mode) is True
    assert _prescan(ids, id_mode) is (fits is not False)
    header = hp.make_header(2, "se_original", 1, "none", id_mode)
    host, kern = IdCodec(header, lib_path=EMU_LIB), IdCodec(header, lib_path=EMU_LIB, device=0)
    a, off = _arrays(ids)
    if fits is None:   # no instrument name: FQSX_E_ARG from both coders, not a staging matter
        for c in (host, kern):
            with pytest.raises(FqsxError, match=r": -1: .*no instrument name") as e:
                c.encode_block(a, off)
            assert e.value.staging is False
        assert kern.error_kind() == 2
    elif fits:
        want = host.encode_block(a, off)
        assert kern.encode_block(a, off) == want and kern.error_kind() == 0
        if b"\0" not in probe:   # (a NUL ends a plain line for the reference's decoder, id.cpp:495-666: such an id does not come back)
            dec = IdCodec(header, lib_path=EMU_LIB, device=0)   # the decoder's staging takes what the encoder's takes
            ref = IdCodec(header, lib_path=EMU_LIB)
            got, want_lines = dec.decode_block(want, len(ids)), ref.decode_block(want, len(ids))
            assert np.array_equal(got[0], want_lines[0]) and np.array_equal(got[1], want_lines[1])
            dec.close(); ref.close()
    else:
        with pytest.raises(FqsxError, match=r": -5: .*staging sizes") as e:
            kern.encode_block(a, off)
        assert e.value.staging is True and kern.error_kind() == 5
        assert len(host.encode_block(a, off)) == 2
    host.close(); kern.close()


@pytest.mark.parametrize("id_mode", ["lossless", "instrument"])
def test_a_refused_block_names_its_reason(built, id_mode):
    """a byte >= 128: FQSX_E_ARG from both coders, each with a message of its own (the host coder sets no error text in the library)"""
    header = hp.make_header(2, "se_original", 1, "none", id_mode)
    a, off = _arrays([b"@ok.1", b"@caf\xe9.2", b"@ok.3", b"@ok.4"])
    kern = IdCodec(header, lib_path=EMU_LIB, device=0)
    with pytest.raises(FqsxError, match="no instrument name" if id_mode == "instrument" else "128-symbol"):
        kern.encode_block(*_arrays([b"@abc/1"] * 4 if id_mode == "instrument" else [b"@\xff.1"] * 4))   # (leaves its text in the library)
    host = IdCodec(header, lib_path=EMU_LIB)
    with pytest.raises(FqsxError, match=r"fqsx_id_encode_block: -1: .*128-symbol alphabet") as e:
        host.encode_block(a, off)
    assert e.value.staging is False
    kern.close()
    kern = IdCodec(header, lib_path=EMU_LIB, device=0)
    with pytest.raises(FqsxError, match=r"fqsx_idg_encode_block: -1: .*128-symbol alphabet") as e:
        kern.encode_block(a, off)
    assert e.value.staging is False and kern.error_kind() == 1
    with pytest.raises(FqsxError, match="odd number of reads"):
        IdCodec(header, lib_path=EMU_LIB).encode_block(*_arrays([b"@ok.1"] * 3), True)
    host.close(); kern.close()


@pytest.mark.parametrize("where", WHERE)
def test_bytes_beyond_the_alphabet_after_the_instrument_name_are_not_coded(where, request):
    """Instrument mode codes the name alone (id.cpp:421-495), so the reference and the host coder take a byte >= 128 behind it.
    The kernel refused such a line (IDK_ERR_BYTE from staging the whole line): found while writing these tests, fixed in
    idk_id_instrument."""
    lib = _lib(where, request)
    ids = [b"@M%d%s%d caf\xe9 \xff%d" % (i % 5, (b".", b" ", b":")[i % 3], i, i) for i in range(200)]
    header = hp.make_header(2, "se_original", 1, "none", "instrument")
    host, kern = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    a, off = _arrays(ids)
    want = host.encode_block(a, off)
    assert kern.encode_block(a, off) == want and kern.error_kind() == 0
    got, _ = IdCodec(header, lib_path=lib, device=0).decode_block(want, len(ids))
    assert got.tobytes() == b"".join(_name_of(x) + b"\n" for x in ids)
    host.close(); kern.close()
    rec = hp.Records(ids, synth_reads(len(ids), 60, 20000, 33), synth_quals(len(ids), 60, 33))
    st = {}
    data = compress_records(rec, 2, "o", 1, lib_path=lib, id_mode="instrument", stats=st)
    assert st["gpu_ids"] is True and data == compress_records(rec, 2, "o", 1, lib_path=lib, id_mode="instrument", gpu_ids=False)


# ---- the inputs of the issue's table: each compresses, to the file the host coder writes --------------------------------------------
TABLE = [("lossless", "an id of 1024 bytes", _long(1024), False), ("lossless", "129 tokens, ','", _tokens_lossless(128, b","), False),
         ("instrument", "a name of 63 bytes", b"@" + b"n" * 62 + b".1", False), ("instrument", "a name of 70 bytes", b"@" + b"n" * 69 + b":1", False),
         ("lossless", "70 colons", b"@" + b"ab:" * 9 + b":" * 61 + b"c" * 61, True)]


@pytest.mark.parametrize("id_mode,what,probe,fits", [pytest.param(*p, id=("%s-%s" % p[:2]).replace(" ", "_")) for p in TABLE])
def test_an_id_on_either_side_of_a_limit_compresses_to_the_host_coders_file(built, id_mode, what, probe, fits):
    ids = [b"@ord.%d x:%d" % (i, 7 * i) for i in range(80)]
    ids[61:61] = [probe, probe]
    rec = hp.Records(ids, synth_reads(len(ids), 60, 20000, 31), synth_quals(len(ids), 60, 31))
    want = compress_records(rec, 2, "o", 1, lib_path=EMU_LIB, id_mode=id_mode, gpu_ids=False)
    st = {}
    assert compress_records(rec, 2, "o", 1, lib_path=EMU_LIB, id_mode=id_mode, stats=st) == want
    assert st["gpu_ids"] is fits and st["id_host_fallback"] is False
    text = fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(len(rec))], [rec.qual_bytes(i) for i in range(len(rec))])
    st = {}
    assert compress_fastq(text, threads=2, order="o", genome_size_mbp=1, quality_mode="none", id_mode=id_mode, lib_path=EMU_LIB, stats=st) == want
    assert st["gpu_ids"] is fits and st["id_host_fallback"] is False


# ---- more instrument names than a worker's list holds: a host-side decision, emulation only ------------------------------------------
def test_4096_names_in_one_worker_stay_on_the_kernel(built):
    header = hp.make_header(1, "se_original", 1, "none", "instrument")
    host, kern = IdCodec(header, lib_path=EMU_LIB), IdCodec(header, lib_path=EMU_LIB, device=0)
    ids = [b"@n%d.%d" % (i, i) for i in range(4096)] + [b"@n%d:1" % ((i * 997) % 4096) for i in range(300)]   # (then codes of four bytes)
    for b in range(0, len(ids), 1099):
        a, off = _arrays(ids[b:b + 1099])
        assert kern.encode_block(a, off) == host.encode_block(a, off), f"block at {b}"
    assert kern.state()[0, 2] == 4096
    host.close(); kern.close()


def test_the_4097th_name_changes_over_to_the_host_coder_in_mid_file(built):
    n = 5000
    ids = [b"@n%d.%d" % (i, i) for i in range(n)]
    rec = hp.Records(ids, synth_reads(n, 60, 20000, 32), synth_quals(n, 60, 32))
    blocks = hp.form_blocks(rec, "se_sorted", exact_ties=True)
    assert sum(len(b) for b in blocks[:-1]) > 4096 and len(blocks[0]) < 4096   # the 4097th name comes in a later block than the first
    want = compress_records(rec, 1, "s", 1, lib_path=EMU_LIB, id_mode="instrument", gpu_ids=False)
    st = {}
    assert compress_records(rec, 1, "s", 1, lib_path=EMU_LIB, id_mode="instrument", stats=st) == want
    assert st["gpu_ids"] is True and st["id_host_fallback"] is True   # (the pre-scan cannot know; the blocks before stay as the kernel wrote them)
    text = fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(n)], [rec.qual_bytes(i) for i in range(n)])
    for resident in (False, True):
        st = {}
        assert compress_fastq(text, threads=1, genome_size_mbp=1, quality_mode="none", lib_path=EMU_LIB, stats=st, resident=resident) == want   # -om s -im i: the defaults
        assert st["gpu_ids"] is True and st["id_host_fallback"] is True
    with pytest.raises(FqsxError, match="more than 4096 instrument names") as e:   # (what the change-over catches)
        kern = IdCodec(hp.make_header(1, "se_original", 1, "none", "instrument"), lib_path=EMU_LIB, device=0)
        try:
            kern.encode_block(*_arrays(ids[:4097]))
        finally:
            kind = kern.error_kind()
            kern.close()
    assert e.value.staging is True and kind == 6
