"""The window-parallel insert phase (fqsx_dev.h: insert_windows) on a real MI355X: window edges, the in-order fall-back
mixed in, saturating counters, draw-heavy inputs of high multiplicity against the oracle, and both paths against each
other.  The switches are read when a codec is created, so every case sets them first."""
import numpy as np
import pytest

from conftest import c1_records, check_against_digest, check_against_fqs, check_decode_fqs
from fqsqueezer_amd import hostpipe as hp

pytestmark = pytest.mark.gpu


def gpu(header):
    from fqsqueezer_amd.codec import DnaCodec
    return DnaCodec(header, device=0)


@pytest.mark.parametrize("name,small", [("c1_10k_s_t4.fqs", False), ("c1_10k_o_t1.fqs", False), ("c1_10k_s_t4.fqs", True)])
def test_windows_of_64_keys(name, small, monkeypatch):
    """Duplicates straddle windows and every phase has many of them; `small`: from 64-slot sub-tables at 85 % load, so that
    claims race into full buckets and down the overflow chain."""
    monkeypatch.setenv("FQSX_INS_WINDOW", "64")
    if small:
        monkeypatch.setenv("FQSX_GTAB_INIT", "64")
        monkeypatch.setenv("FQSX_TAB_LOAD_PCT", "85")
    codec = check_against_fqs(gpu, c1_records(), name)
    st = codec.stats()
    assert st["ins_windows"] > 1000, st
    check_decode_fqs(gpu, c1_records(), name)


def test_in_order_windows_mixed_in(monkeypatch):
    """A multiplicity cap of 1: every window that holds a k-mer twice goes through the in-order routine, the others do not."""
    monkeypatch.setenv("FQSX_INS_WINDOW", "64")
    monkeypatch.setenv("FQSX_INS_MAXMULT", "1")
    st = check_against_fqs(gpu, c1_records(), "c1_10k_s_t4.fqs").stats()
    assert st["ins_windows_in_order"] > 0 and st["ins_windows"] > 0, st


@pytest.mark.parametrize("om", ["s", "o"])
def test_saturated_counters_in_windows_of_64(om, monkeypatch):
    """c13: draws on s-mers, counters at their maxima (where a window cannot be decided ahead and goes in order)."""
    monkeypatch.setenv("FQSX_INS_WINDOW", "64")
    st = check_against_digest(gpu, f"c13_sat_{om}_t4.json").stats()
    assert st["ins_windows"] > 0, st


# ---- draw-heavy inputs of high multiplicity against the oracle: T = 7, -gs 1, eight blocks of the sorted file ----------
def _genome_2k():
    from fqsqueezer_amd.synth import synth_reads
    return synth_reads(3000, 100, 2000, 29)   # counters pass the thresholds within a few blocks; several twists per phase


def _copies_and_poly_a():
    from fqsqueezer_amd.synth import synth_reads
    one = synth_reads(1, 100, 5000, 31)
    return np.concatenate([np.repeat(one, 400, axis=0), np.full((50, 100), ord("A"), dtype=np.uint8)])


_INPUTS = {"genome_2k": _genome_2k, "copies_and_poly_a": _copies_and_poly_a}
_cache = {}


def _blocks_and_oracle(which):
    """the input's first eight blocks and the oracle's streams of them, computed once"""
    if which not in _cache:
        from oracle.pyoracle import OracleCodec
        reads = _INPUTS[which]()
        rec = hp.Records([b"@r%d" % i for i in range(len(reads))], reads, reads)
        header = hp.make_header(7, "se_sorted", 1)
        order = np.concatenate(hp.sorted_order(rec))
        B = len(order) // 8
        blocks = [hp.block_arrays(rec, order[lo:lo + B]) for lo in range(0, 8 * B, B)]
        cpu = OracleCodec(header)
        _cache[which] = (header, blocks, [cpu.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)])
    return _cache[which]


def _encode(header, blocks):
    codec = gpu(header)
    return [codec.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)], codec


@pytest.mark.parametrize("window", [None, "64"])
@pytest.mark.parametrize("which", ["genome_2k", "copies_and_poly_a"])
def test_draw_heavy_inputs_match_the_oracle(which, window, monkeypatch):
    if window:
        monkeypatch.setenv("FQSX_INS_WINDOW", window)
    header, blocks, want = _blocks_and_oracle(which)
    got, codec = _encode(header, blocks)
    for g in range(len(blocks)):
        assert got[g] == want[g], f"{which}: block {g} differs from the oracle"
    st = codec.stats()
    assert st["ins_windows"] > 0, st


def test_parallel_and_in_order_paths_agree(monkeypatch):
    header, blocks, want = _blocks_and_oracle("genome_2k")
    par, c_par = _encode(header, blocks)
    monkeypatch.setenv("FQSX_INS_PARALLEL", "0")
    ser, c_ser = _encode(header, blocks)
    assert par == ser == want
    a, b = c_par.capacity(), c_ser.capacity()
    assert (a["smers"], a["bmers"], a["growths"]) == (b["smers"], b["bmers"], b["growths"])
    assert c_par.stats()["ins_windows"] > 0 and c_ser.stats()["ins_windows"] == 0 and c_ser.stats()["ins_windows_in_order"] == 0
