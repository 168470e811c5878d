"""Quality stream: oracle restatement, emulated kernel and HIP kernel (k_qual_encode, csrc/fqsx_qual.h)
against the reference's quality streams (all four quality modes, single- and paired-end).

What pins what:
  c8_qual_*       the reference's streams for fixed 100 bp reads at T = 3 / 4: the plain path of every mode, SE and PE.
  c27_halving_*   40 000 x 30 bp at T = 1: position 0's model passes 2^15 and is halved -- in the 96- / 8- / 4- / 2-symbol slot
                  layouts, with the total in a word of its own (N = 96, 8, 4) and in the statistics' word (N = 2).
  c27_windows_*   read lengths on both sides of every edge of the LDS staging windows (4032 positions plus the 64 before
                  them) and of the 64-symbol chunks, one worker and three.
  c27_alphabet_*  quality symbols 0 .. 93 in ragged reads: every bin of the three quantisers and its borders; in lossless
                  mode `cum` sums over all 24 words of a model.
  c23_*.fqs       the reference's own streams, worker by worker, for ragged reads in the lossy modes and for pairs.
  OracleQual      inputs made here, one codec instance over six blocks (the table grows, the models persist), T up to 255,
                  empty reads, one-symbol reads, fewer reads than workers: no reference file, but the oracle is pinned to the
                  reference by every digest above, and unlike a round trip it shares no code with the kernel.
Each comparison runs for the oracle (digests), the emulation build (one lane) and, marked gpu, device 0 (64 lanes: the
hardware reciprocal, the cross-lane hand-over of the model values, the compare-and-swap slot claims, the packed-word updates).
tests/test_rc_device.py holds the range coder itself; tests/test_fqs_file.py whole files where most workers have no read."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records, check_quality_digest
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.synth import C27, synth_c27

CASES = ["c8_qual_o_t4.json", "c8_qual_8_t4.json", "c8_qual_4_t4.json", "c8_qual_2_t4.json", "c8_qual_pe8_t3.json"]
WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("name", CASES)
def test_oracle_quality_matches_reference(name):
    from oracle.pyoracle import OracleQual
    check_quality_digest(OracleQual, name)


@pytest.mark.parametrize("name", CASES)
def test_emu_quality_matches_reference(built, name):
    from fqsqueezer_amd.codec import QualCodec
    check_quality_digest(lambda h: QualCodec(h, lib_path=EMU_LIB), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_quality_matches_reference(name):
    from fqsqueezer_amd.codec import QualCodec
    check_quality_digest(lambda h: QualCodec(h, device=0), name)


def _make_codec(where, request):
    from fqsqueezer_amd.codec import QualCodec
    if where == "emu":
        request.getfixturevalue("built")
        return lambda h: QualCodec(h, lib_path=EMU_LIB)
    return lambda h: QualCodec(h, device=0)


# ---- the c27 digests: halving, staging windows, whole alphabet -----------------------------------------------------------------
_c27_inputs = {}


def _c27_blocks(name):
    """[(quals, off)] per container block of a c27 input (made once)"""
    if name not in _c27_inputs:
        rec = hp.Records(*synth_c27(name))
        _c27_inputs[name] = [hp.qual_arrays(rec, idx) for idx in hp.form_blocks(rec, "se_original")]
    return _c27_inputs[name]


def check_c27_digest(make_codec, tag):
    d = json.load(open(os.path.join(GOLD, tag + ".json")))
    name, qm, t = C27[tag]
    assert (d["input"], d["qm"], d["threads"]) == (name, qm, t)
    header = bytes.fromhex(d["header"])
    assert header[4] == t and header[8] == 20
    blocks = _c27_blocks(name)
    assert len(blocks) == d["n_blocks"]
    codec = make_codec(header)
    for g, ((q, off), ref) in enumerate(zip(blocks, d["blocks"])):
        assert len(off) - 1 == ref["n_reads"]
        streams = codec.encode_block(q, off)
        h = hashlib.sha256()
        for s in streams:
            h.update(s)
        assert sum(len(s) for s in streams) == ref["bytes"] and h.hexdigest() == ref["sha256"], f"{tag}: block {g} quality stream differs from the reference"


def test_c27_inputs_reach_what_they_are_for():
    """position 0 is coded more than 2^15 times by the one worker; the window reads straddle 4032 and its multiples; every symbol occurs"""
    assert len(_c27_blocks("halving")) == 1 and len(_c27_blocks("halving")[0][1]) - 1 == 40000 > (1 << 15) + 96
    lens = np.diff(_c27_blocks("windows")[0][1].astype(np.int64)).tolist()
    assert {4031, 4032, 4033, 4095, 4096, 4097, 8063, 8064, 8065, 63, 64, 65, 12100} <= set(lens)
    q = np.concatenate([b[0] for b in _c27_blocks("alphabet")])
    assert set(np.unique(q).tolist()) == set(range(33, 33 + 94))


@pytest.mark.parametrize("tag", sorted(C27))
def test_oracle_quality_matches_reference_at_the_edges(tag):
    from oracle.pyoracle import OracleQual
    check_c27_digest(OracleQual, tag)


@pytest.mark.parametrize("tag", sorted(C27))
def test_emu_quality_matches_reference_at_the_edges(built, tag):
    from fqsqueezer_amd.codec import QualCodec
    check_c27_digest(lambda h: QualCodec(h, lib_path=EMU_LIB), tag)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(C27))
def test_hip_quality_matches_reference_at_the_edges(tag):
    from fqsqueezer_amd.codec import QualCodec
    check_c27_digest(lambda h: QualCodec(h, device=0), tag)


# ---- the reference's own streams for ragged reads and pairs, worker by worker ---------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["c23_c4_q8_t4", "c23_c4_q4_t4", "c23_c4_q2_t4", "c23_c5_pe_qo_t3"])
def test_encoder_writes_the_reference_streams_of_ragged_and_paired_reads(where, request, name):
    """the inputs of the c23 files (c4: ragged reads in the lossy modes, T = 4; 1400 c5 pairs, lossless, -om s, T = 3) encoded
    block by block: every worker's stream is byte for byte the one in the reference's file"""
    d = json.load(open(os.path.join(GOLD, name + ".json")))
    header, blocks = hp.parse_fqs(open(os.path.join(GOLD, name + ".fqs"), "rb").read())
    T = header[4]
    if d.get("paired"):
        r1, r2 = (hp.Records(r.ids[:d["pairs"]], r.seq[:d["pairs"]], r.qual[:d["pairs"]]) for r in c5_records())
        arrays = [hp.qual_arrays_pe(r1, r2, idx) for idx in hp.form_blocks_pe(r1, r2, "pe_sorted")]
    else:
        rec = c4_records()
        arrays = [hp.qual_arrays(rec, idx) for idx in hp.form_blocks(rec, "se_original")]
    assert len(arrays) == len(blocks)
    codec = _make_codec(where, request)(header)
    for g, ((q, off), ref) in enumerate(zip(arrays, blocks)):
        assert len(off) - 1 == ref.n_reads
        got = codec.encode_block(q, off)
        for w in range(T):
            assert got[w] == ref.streams[w][hp.STREAM_QUALITY], f"{name}: block {g} worker {w} differs from the reference's stream"


# ---- the kernel against the oracle on inputs made here --------------------------------------------------------------------------
def _six_blocks(family):
    from test_quality_decode import _blocks_fixed, _blocks_paired
    if family == "fixed":
        return _blocks_fixed(6, 448, 100, 41)
    if family == "paired":
        return _blocks_paired(6, 224, 31)
    rng = np.random.default_rng(5)   # the blocks of test_round_trip_empty_and_one_symbol_strings_and_fewer_reads_than_workers, and a sixth
    blocks = []
    for lens in ([0, 1, 0, 0, 1, 1, 7, 0, 1, 130, 0, 65, 64, 63, 1], [1, 0, 3], [0, 0, 0, 0], [1], [9, 0, 8, 1, 200], [1, 1, 0, 64, 1, 5000, 0, 2]):
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        blocks.append((rng.choice(np.frombuffer(b"#-5<AFI", dtype=np.uint8), int(off[-1])), off))
    return blocks


_oracle_streams = {}


def _oracle_six(family, mode, T):
    """the oracle's streams of the six blocks (computed once per case, shared by the emu and the gpu test)"""
    key = (family, mode, T)
    if key not in _oracle_streams:
        from oracle.pyoracle import OracleQual
        header = hp.make_header(T, "pe_original" if family == "paired" else "se_original", 1, mode, "none", 25)
        o = OracleQual(header)
        _oracle_streams[key] = (header, [o.encode_block(q, off) for q, off in _six_blocks(family)])
    return _oracle_streams[key]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("family", ["fixed", "paired", "tiny"])
@pytest.mark.parametrize("T", [1, 3, 64, 255])
@pytest.mark.parametrize("mode", ["lossless", "illumina_8", "illumina_4", "binary"])
def test_encoder_equals_the_oracle_over_six_blocks(where, request, mode, T, family):
    """one encoder over six blocks -- 448 x 100, paired ragged mates, or empty / one-symbol reads and fewer reads than workers --
    writes the oracle's streams, worker by worker"""
    header, want = _oracle_six(family, mode, T)
    codec = _make_codec(where, request)(header)
    slots0 = codec.contexts()["slots_per_worker"]
    for b, ((q, off), ref) in enumerate(zip(_six_blocks(family), want)):
        got = codec.encode_block(q, off)
        assert len(got) == T
        bad = [w for w in range(T) if got[w] != ref[w]]
        assert not bad, f"block {b}: workers {bad[:8]} differ from the oracle"
    if family != "tiny" and T == 1:
        assert codec.contexts()["slots_per_worker"] > slots0, "the context table never grew"
