"""Deferred coding on a real MI355X: in the phases of a single-end sorted block that are followed by another phase the
encode launch leaves its coding-queue entries in device memory, and k_code_se_sorted runs the models and the range coder
over them on the codec's second stream.  Everything is compared byte for byte with the reference goldens or the oracle.
FQSX_DEFER_CODING, FQSX_TEST_GQ_CAP and FQSX_PROTO_DEBUG are read when a codec is created, so a case that sets one does
so first."""
import threading

import numpy as np
import pytest

from conftest import c1_records, check_against_fqs
from fqsqueezer_amd import hostpipe as hp
from test_gpu_insert_parallel import _blocks_and_oracle   # (inputs and the oracle's streams of them, computed once)

pytestmark = pytest.mark.gpu

CQ_FULL = 10   # FQSX_ERR_CQ_FULL (fqsx_layout.h)
# Counters of probe work, which depend on which wave got to a look-up first and differ between two runs of ONE mode on one
# input (profiles/defer_coding_stats_runs.txt, three runs each of this file's genome_2k case: gprobe 671574 / 671591, lprobe
# 62605 / 62622 in either mode, gslot, lslot and gins_slot different in nearly every run); every other counter is a function
# of the input and must not move -- between the modes or between two runs of one (test_both_modes_agree checks both).
WAVE_TIMING_COUNTERS = ("gprobe", "gslot", "lprobe", "lslot", "gins_slot")


def gpu(header):
    from fqsqueezer_amd.codec import DnaCodec
    return DnaCodec(header, device=0)


def deferred_segments(n_reads, T, generation):
    """block_prepare's schedule: S synchronisation points, each of them a phase that is followed by another one"""
    S = min(100 - generation, n_reads // T // 2) if generation < 100 else 0
    return max(S - 1, 0)


# ---- 1. goldens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_10k_s_t4.fqs", "c1_10k_s_t1.fqs"])
def test_goldens_through_the_deferred_path(name):
    codec = check_against_fqs(gpu, c1_records(), name)
    assert codec.kernel_times()["other_launches"] >= 24   # (dozens of deferred segments at generation 0: the path was taken)


# ---- 2. both modes ---------------------------------------------------------------------------------------------------
def test_both_modes_agree(monkeypatch):
    header, blocks, want = _blocks_and_oracle("genome_2k")

    def run(switch):
        monkeypatch.setenv("FQSX_DEFER_CODING", switch)
        codec = gpu(header)
        return [codec.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)], codec

    new, c_new = run("1")
    old, c_old = run("0")
    again, c_again = run("1")
    assert new == want, "deferred coding differs from the oracle"
    assert old == want, "the combined launches differ from the oracle"
    assert again == want
    s_new, s_old, s_again = c_new.stats(), c_old.stats(), c_again.stats()
    for s in (s_new, s_old, s_again):
        for k in ("timers",) + WAVE_TIMING_COUNTERS:
            s.pop(k)
    assert len(s_new) >= 11
    assert s_new == s_old
    assert s_new == s_again   # (the counters compared are the ones that two runs of one mode agree on)
    k_new, k_old = c_new.kernel_times(), c_old.kernel_times()
    assert k_new["encode_launches"] == k_old["encode_launches"] > 0
    n_deferred = sum(deferred_segments(len(off) - 1, header[4], g) for g, (_, off) in enumerate(blocks))
    assert n_deferred > 0
    assert c_new.capacity()["growths"] == 0   # (no phase was run twice: the count below is the schedule's)
    assert k_new["other_launches"] - k_old["other_launches"] == n_deferred, (k_new, k_old, n_deferred)


# ---- 3. growth posted while a coding kernel is in flight ---------------------------------------------------------------
def test_growth_posted_beside_a_coding_kernel(monkeypatch):
    """the posted phase's symbols are coded all the same, the skipped launches leave stale tags behind, and the recovery
    takes up behind both streams"""
    monkeypatch.setenv("FQSX_GTAB_INIT", "64")
    monkeypatch.setenv("FQSX_TAB_LOAD_PCT", "85")
    codec = check_against_fqs(gpu, c1_records(), "c1_10k_s_t4.fqs")
    assert codec.capacity()["growths"] > 0


# ---- 4. schedule edges -------------------------------------------------------------------------------------------------
def _reads_150(n, seed):
    from fqsqueezer_amd.synth import synth_reads
    reads = synth_reads(n, 150, 3000, seed)
    rec = hp.Records([b"@e%d" % i for i in range(n)], reads, reads)
    return hp.block_arrays(rec, np.concatenate(hp.sorted_order(rec)))


_edges = {}


def _edge_blocks():
    """T = 8.  Sequence "sizes": 32 reads (S = 1: one deferred and one combined segment), 24 reads (S = 0: the second stream and
    the queues go back), 5 reads (workers without reads; S = 0 again -- a block with a deferred phase gives every worker at least
    four reads and every deferred phase of a worker at least one, so a coding kernel never meets a worker whose launch ran and
    queued nothing; the queues it finds empty are those of skipped launches, test_growth_posted_beside_a_coding_kernel).
    Sequence "generations": blocks of 32 reads at generations 98, 99, 100 -- S falls from 1 to 0."""
    if not _edges:
        from oracle.pyoracle import OracleCodec
        header = hp.make_header(8, "se_sorted", 1)
        for name, sizes, gens in (("sizes", (32, 24, 5), (0, 1, 2)), ("generations", (32, 32, 32), (98, 99, 100))):
            blocks = [_reads_150(n, 40 + k) for k, n in enumerate(sizes)]
            cpu = OracleCodec(header)
            _edges[name] = (header, blocks, gens, [cpu.encode_block(b, o, g) for (b, o), g in zip(blocks, gens)])
    return _edges


@pytest.mark.parametrize("name", ["sizes", "generations"])
def test_schedule_edges(name):
    header, blocks, gens, want = _edge_blocks()[name]
    codec = gpu(header)
    coded = []
    for (bases, off), g, w in zip(blocks, gens, want):
        assert codec.encode_block(bases, off, g) == w, f"{name}: generation {g} differs from the oracle"
        coded.append(codec.kernel_times()["other_launches"])
    # one coding kernel, for the first block's one deferred segment; never one for a block without a second phase
    assert coded == [1, 1, 1], coded
    assert [deferred_segments(len(off) - 1, 8, g) for (_, off), g in zip(blocks, gens)] == [1, 0, 0]
    codec.close()   # (straight behind the last block)


# ---- 5. the resolving wave's fall-back branches push into the queue in device memory too ---------------------------------
@pytest.mark.parametrize("dbg", [1, 2, 4], ids=["scouts_off", "abandon_every_3rd_read", "window_after_every_chunk"])
def test_fall_back_branches(dbg, monkeypatch):
    monkeypatch.setenv("FQSX_PROTO_DEBUG", str(dbg))
    header, blocks, want = _blocks_and_oracle("genome_2k")
    codec = gpu(header)
    assert codec.encode_block(*blocks[0], 0) == want[0]
    assert codec.kernel_times()["other_launches"] == deferred_segments(len(blocks[0][1]) - 1, header[4], 0) > 0


# ---- 6. capacity -------------------------------------------------------------------------------------------------------
_dense = {}


def _dense_block():
    """The most queue entries per base: reads of 20 bp (the shortest any golden of the project carries -- the format itself names
    no minimum; a read's head costs its triples whatever its length) next to reads that are runs of N, T = 4, 24 phases."""
    if not _dense:
        from oracle.pyoracle import OracleCodec
        rng = np.random.Generator(np.random.PCG64(5))
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=600)]
        seqs = []
        for i in range(200):
            if i % 5 == 4:
                seqs.append(b"N" * int(rng.integers(20, 60)))
            else:
                p = int(rng.integers(0, 580))
                s = genome[p:p + 20].copy()
                if i % 7 == 0:
                    s[int(rng.integers(0, 20)):][:6] = ord("N")
                seqs.append(s.tobytes())
        rec = hp.Records([b"@d%d" % i for i in range(len(seqs))], seqs, seqs)
        header = hp.make_header(4, "se_sorted", 1)
        block = hp.block_arrays(rec, np.concatenate(hp.sorted_order(rec)))
        _dense.update(header=header, block=block, want=OracleCodec(header).encode_block(*block, 0))
    return _dense["header"], _dense["block"], _dense["want"]


@pytest.mark.parametrize("cap", [None, "0"], ids=["sized_by_the_host", "exactly_the_bound"])
def test_capacity_holds_the_densest_reads(cap, monkeypatch):
    """FQSX_TEST_GQ_CAP=0: the queues hold exactly bases + reads x FQSX_HD_RAW of the largest deferred phase, without the slack
    block_prepare adds -- one entry more than the bound in any phase of any worker fails the block (FQSX_ERR_CQ_FULL)"""
    if cap is not None:
        monkeypatch.setenv("FQSX_TEST_GQ_CAP", cap)
    header, block, want = _dense_block()
    codec = gpu(header)
    assert codec.encode_block(*block, 0) == want
    assert codec.kernel_times()["other_launches"] == deferred_segments(200, 4, 0) == 24


def test_a_queue_too_small_fails_the_block(monkeypatch):
    from fqsqueezer_amd.codec import FqsxError
    monkeypatch.setenv("FQSX_TEST_GQ_CAP", "8")
    header, block, _ = _dense_block()
    codec = gpu(header)
    streams = None
    with pytest.raises(FqsxError, match=f"device error {CQ_FULL} "):
        streams = codec.encode_block(*block, 0)
    assert streams is None


# ---- 7. two codecs in two threads on one device --------------------------------------------------------------------------
def test_two_codecs_in_two_threads():
    header, blocks, want = _blocks_and_oracle("genome_2k")
    lone = gpu(header)
    alone = [lone.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks[:4])]
    assert alone == want[:4]
    out, errs = [None, None], []

    def work(k):
        try:
            codec = gpu(header)   # (its own second stream)
            out[k] = [codec.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks[:4])]
            codec.close()
        except Exception as e:   # noqa: BLE001 -- reported by the asserting thread
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert out[0] == alone and out[1] == alone
