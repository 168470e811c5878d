"""Quality-stream decoder (k_qual_decode, csrc/fqsx_qdec.h) and its C ABI: the reference's own quality streams decode to the
reference decoder's output, and encode -> decode through the library's encoder (which tests/test_quality.py pins to the
reference) is exact, with the decoder's context table ending equal to the encoder's.  Every case runs on the emulation build
(a 1-lane wave: coder, table, partition, bounds) and, marked gpu, on device 0 (the cross-lane search, the look-ahead, the
word-gathered output)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records, c10_records, c20_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.synth import synth_quals

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]

# quality_code_map_fwd / _rev of the reference, quality.cpp:84-149 (index = quality - 33)
FWD8 = [0] * 2 + [1] * 8 + [2] * 10 + [3] * 5 + [4] * 5 + [5] * 5 + [6] * 5 + [7] * 56
REV8 = [0, 6, 15, 22, 27, 33, 37, 40]
FWD4 = [0] * 2 + [1] * 13 + [2] * 16 + [3] * 65
REV4 = [0, 12, 23, 37]


def quantised(q: np.ndarray, mode: str, thr: int = 20) -> np.ndarray:
    """what the reference's decoder returns for qualities q (ASCII): rev[fwd[q - 33]] + 33"""
    q = np.asarray(q, dtype=np.uint8)
    if mode == "lossless":
        return q
    if mode == "binary":
        fwd, rev = [0] * thr + [1] * (96 - thr), [0, thr]
    else:
        fwd, rev = (FWD8, REV8) if mode == "illumina_8" else (FWD4, REV4)
    assert len(fwd) == 96
    table = np.array([rev[f] + 33 for f in fwd], dtype=np.uint8)
    return table[q - 33]


MODE_OF = {0: "lossless", 1: "illumina_8", 2: "illumina_4", 3: "binary"}


def _codec(where, request):
    from fqsqueezer_amd.codec import MetaCodec, QualCodec
    if where == "emu":
        request.getfixturevalue("built")
        return (lambda h: QualCodec(h, lib_path=EMU_LIB)), (lambda t: MetaCodec(t, lib_path=EMU_LIB))
    return (lambda h: QualCodec(h, device=0)), (lambda t: MetaCodec(t))


# ---- 1. streams written by the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_reference_lossless_file_streams_decode_to_the_input(where, request):
    """c10_full_o_t3.fqs (-om o -t 3 -qm o -im o): every block's quality streams -> the input qualities, its meta streams -> the
    input read lengths"""
    mkq, mkm = _codec(where, request)
    rec = c10_records()
    header, blocks = hp.parse_fqs(open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read())
    blks = hp.form_blocks(rec, "se_original")
    assert len(blks) == len(blocks)
    qc, mc = mkq(header), mkm(header[4])
    for idx, ref in zip(blks, blocks):
        want, off = hp.qual_arrays(rec, idx)
        lens = mc.decode_block([ref.streams[w][hp.STREAM_META] for w in range(header[4])], ref.n_reads)
        assert np.array_equal(lens, np.diff(off.astype(np.int64)))
        got = qc.decode_block([ref.streams[w][hp.STREAM_QUALITY] for w in range(header[4])], off)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["c23_c4_q8_t4", "c23_c4_q4_t4", "c23_c4_q2_t4", "c23_c5_pe_qo_t3"])
def test_reference_files_decode_to_what_the_reference_decoder_writes(where, request, name):
    """the reference's files in the lossy modes (c4: ragged reads, T = 4) and a paired lossless one (the first 1400 c5 pairs, -om s, T = 3):
    meta -> read lengths, quality -> rev[fwd[q]] of the input, and the decoded quality lines hash to the digest of the lines
    `fqs d` wrote for the file (tools/make_golden.py c23)"""
    mkq, mkm = _codec(where, request)
    d = json.load(open(os.path.join(GOLD, name + ".json")))
    header, blocks = hp.parse_fqs(open(os.path.join(GOLD, name + ".fqs"), "rb").read())
    T, mode, paired = header[4], MODE_OF[header[6]], header[5] >= 2
    assert T == d["threads"] and bool(d.get("paired")) == paired
    if paired:
        r1, r2 = (hp.Records(r.ids[:d["pairs"]], r.seq[:d["pairs"]], r.qual[:d["pairs"]]) for r in c5_records())
        blks = hp.form_blocks_pe(r1, r2, "pe_sorted")
        arrays = lambda idx: hp.qual_arrays_pe(r1, r2, idx)   # noqa: E731
    else:
        rec = c4_records()
        blks = hp.form_blocks(rec, "se_original")
        arrays = lambda idx: hp.qual_arrays(rec, idx)   # noqa: E731
    assert len(blks) == len(blocks)
    qc, mc = mkq(header), mkm(T)
    h1, h2, n = hashlib.sha256(), hashlib.sha256(), 0
    for idx, ref in zip(blks, blocks):
        q, off = arrays(idx)
        lens = mc.decode_block([ref.streams[w][hp.STREAM_META] for w in range(T)], ref.n_reads, paired)
        assert np.array_equal(lens, np.diff(off.astype(np.int64)))
        got = qc.decode_block([ref.streams[w][hp.STREAM_QUALITY] for w in range(T)], off)
        assert np.array_equal(got, quantised(q, mode, header[8]))
        n += ref.n_reads
        for r in range(ref.n_reads):
            (h2 if paired and r & 1 else h1).update(got[int(off[r]):int(off[r + 1])].tobytes() + b"\n")
    assert n == d["decoded_reads"]
    assert h1.hexdigest() == d["decoded_quality_sha256"]
    if paired:
        assert h2.hexdigest() == d["decoded_quality_sha256_mate2"]


# ---- 2. round trips against the library's encoder ---------------------------------------------------------------------------
def _round_trip(mkq, header, blocks, thr=20):
    """blocks of (quals, off) through ONE encoder and ONE decoder; returns the decoder's slots per worker before / after"""
    enc, dec = mkq(header), mkq(header)
    mode = MODE_OF[header[6]]
    slots0 = dec.contexts()["slots_per_worker"]
    for b, (q, off) in enumerate(blocks):
        got = dec.decode_block(enc.encode_block(q, off), off)
        assert np.array_equal(got, quantised(q, mode, thr)), f"block {b} decoded wrongly"
        ce, cd = enc.contexts(), dec.contexts()
        assert ce["per_worker"] == cd["per_worker"], f"block {b}: the decoder stored other contexts than the encoder"
    return slots0, dec.contexts()["slots_per_worker"]


def _blocks_fixed(n_blocks, n_reads, L, seed):
    return [(synth_quals(n_reads, L, seed + b).reshape(-1), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)) for b in range(n_blocks)]


def _blocks_paired(n_blocks, n_pairs, seed):
    """mates of different lengths, interleaved (the quality coder sees a paired block as 2 n reads; the worker partition keeps pairs together)"""
    out = []
    for b in range(n_blocks):
        rng = np.random.default_rng(seed + b)
        lens = np.empty(2 * n_pairs, dtype=np.int64)
        lens[0::2], lens[1::2] = rng.integers(60, 130, n_pairs), rng.integers(30, 100, n_pairs)
        off = np.zeros(2 * n_pairs + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        out.append((synth_quals(1, int(off[-1]), seed + 100 + b).reshape(-1), off))
    return out


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("mode", ["lossless", "illumina_8", "illumina_4", "binary"])
def test_round_trip_many_blocks_one_instance(where, request, mode, T, paired):
    mkq, _ = _codec(where, request)
    header = hp.make_header(T, "pe_original" if paired else "se_original", 1, mode, "none", 25)
    blocks = _blocks_paired(8, 224, 31) if paired else _blocks_fixed(8, 448, 100, 41)
    slots0, slots1 = _round_trip(mkq, header, blocks, thr=25)
    assert slots1 > slots0, "the context table never grew: the models did not persist across a growth"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("mode", ["lossless", "illumina_8"])
def test_round_trip_reads_of_5000_symbols(where, request, mode):
    mkq, _ = _codec(where, request)
    r1, r2 = c20_records()
    q, off = hp.qual_arrays_pe(r1, r2, np.arange(len(r1)))
    _round_trip(mkq, hp.make_header(3, "pe_original", 1, mode), [(q, off), (q[::-1].copy(), off)])


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("T", [1, 4, 64])
def test_round_trip_empty_and_one_symbol_strings_and_fewer_reads_than_workers(where, request, T):
    mkq, _ = _codec(where, request)
    rng = np.random.default_rng(5)
    blocks = []
    for lens in ([0, 1, 0, 0, 1, 1, 7, 0, 1, 130, 0, 65, 64, 63, 1], [1, 0, 3], [0, 0, 0, 0], [1], [9, 0, 8, 1, 200]):
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        blocks.append((rng.choice(np.frombuffer(b"#-5<AFI", dtype=np.uint8), int(off[-1])), off))
    for mode in ("lossless", "illumina_4"):
        _round_trip(mkq, hp.make_header(T, "se_original", 1, mode), blocks)


@pytest.mark.parametrize("where", WHERE)
def test_round_trip_lossless_whole_alphabet(where, request):
    """qualities '!'..'~' (symbols 0..93), skewed towards the top so that contexts repeat: symbols >= 64 are the second
    statistic a lane holds"""
    mkq, _ = _codec(where, request)
    blocks = []
    for b in range(4):
        rng = np.random.default_rng(70 + b)
        n, L = 300, 120
        sym = np.where(rng.random(n * L) < 0.15, rng.integers(0, 94, n * L), 93 - np.minimum(rng.geometric(0.25, n * L) - 1, 93))
        assert sym.min() == 0 and sym.max() == 93 and (sym >= 64).mean() > 0.5
        blocks.append(((sym + 33).astype(np.uint8), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)))
    _round_trip(mkq, hp.make_header(3, "se_original", 1, "lossless"), blocks)


# ---- 3. the halving of a model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_round_trip_through_a_model_halving(where, request):
    """T = 1, binary mode, 40 000 reads of one symbol: position 0 always has the same context, whose total starts at 2 and
    reaches 2^15 after 32 766 symbols"""
    mkq, _ = _codec(where, request)
    rng = np.random.default_rng(9)
    n = 40000
    q = np.where(rng.random(n) < 0.2, 33 + 10, 33 + 30).astype(np.uint8)
    _round_trip(mkq, hp.make_header(1, "se_original", 1, "binary", "none", 20), [(q, np.arange(n + 1, dtype=np.uint64))], thr=20)


# ---- 6. malformed input: the emulation build only (nothing malformed is handed to a GPU) --------------------------------------
def _decode_guarded(built, header, streams, off):
    """fqsx_qual_decode_block into the middle of a guarded buffer; returns (rc, decoded bytes)"""
    import ctypes as C
    from fqsqueezer_amd.codec import QualCodec
    qc = QualCodec(header, lib_path=EMU_LIB)
    T, total = header[4], int(off[-1])
    buf = np.full(total + 128, 0xA5, dtype=np.uint8)
    arr = (C.c_char_p * T)(*[bytes(s) for s in streams])
    lens = np.array([len(s) for s in streams], dtype=np.uint64)
    rc = qc._lib.fqsx_qual_decode_block(qc._h, arr, lens.ctypes.data, off.ctypes.data, len(off) - 1, buf[64:].ctypes.data)
    assert (buf[:64] == 0xA5).all() and (buf[64 + total:] == 0xA5).all(), "bytes outside the block's output range were written"
    return rc, buf[64:64 + total]


@pytest.mark.parametrize("mode", ["lossless", "illumina_8"])
def test_malformed_streams_fail_cleanly(built, mode):
    from fqsqueezer_amd.codec import QualCodec
    header = hp.make_header(3, "se_original", 1, mode)
    q, off = _blocks_fixed(1, 90, 100, 3)[0]
    good = QualCodec(header, lib_path=EMU_LIB).encode_block(q, off)
    rc, out = _decode_guarded(built, header, good, off)
    assert rc == 0 and np.array_equal(out, quantised(q, mode))
    # a stream of 7 bytes / of no bytes for a worker that has reads: refused on the host
    for cut in (7, 0):
        rc, _ = _decode_guarded(built, header, [good[0], good[1][:cut], good[2]], off)
        assert rc == -1   # FQSX_E_ARG
    # cut in the middle: the missing bytes read as 0 -- an error code or wrong symbols, the other workers' reads intact
    rc, out = _decode_guarded(built, header, [good[0], good[1][:len(good[1]) // 2], good[2]], off)
    assert rc in (0, -5)
    if rc == 0:
        (f0, l0), (f1, l1), (f2, l2) = hp.partition_for_workers(90, 3)
        want = quantised(q, mode)
        assert np.array_equal(out[:int(off[l0])], want[:int(off[l0])]) and np.array_equal(out[int(off[f2]):], want[int(off[f2]):])
        assert not np.array_equal(out, want)
    # bytes that are no range-coder stream at all
    junk = np.random.default_rng(1).integers(0, 256, 4000, dtype=np.uint8).tobytes()
    rc, _ = _decode_guarded(built, header, [junk, b"\xff" * 900, junk[::-1]], off)
    assert rc in (0, -5)
    # read offsets that do not ascend
    bad = off.copy()
    bad[5] = bad[7]
    rc, _ = _decode_guarded(built, header, good, bad)
    assert rc == -1


# ---- 7. the kernel is in the product library --------------------------------------------------------------------------------
def test_library_contains_the_quality_decode_kernel():
    import __graft_entry__ as g
    blob = open(g.build_hip(), "rb").read()
    assert b"k_qual_decode" in blob and b"gfx950" in blob
