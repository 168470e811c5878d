"""The mailbox partition at the sender (k_part_sender) and the insert kernel that reads the owners' keys from the sources'
own stretches and decides about growth itself, on a real MI355X: the goldens through the new path, growth posted by the
insert kernel and the recovery behind it, one (source, owner) cell that holds nearly everything, more owners than a wave
has lanes with sources that push nothing, lists of many rounds, and the old three-kernel path against the new one.
FQSX_PART_SENDER is read when a codec is created, so a case that sets it does so first."""
import numpy as np
import pytest

from conftest import c1_records, c5_records, check_against_fqs, check_against_fqs_pe, check_decode_fqs
from fqsqueezer_amd import hostpipe as hp
from test_gpu_insert_parallel import _blocks_and_oracle   # (the draw-heavy inputs and the oracle's streams of them, computed once)

pytestmark = pytest.mark.gpu


def gpu(header):
    from fqsqueezer_amd.codec import DnaCodec
    return DnaCodec(header, device=0)


# ---- goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_10k_s_t4.fqs", "c1_10k_o_t1.fqs"])
def test_single_end_goldens(name):
    check_against_fqs(gpu, c1_records(), name)


def test_paired_end_golden():
    check_against_fqs_pe(gpu, c5_records(), "c5_pe4k_s_t4.fqs")


def test_decoder_still_meets_the_encoder():
    """the decode route keeps the grouped partition; it has to arrive at the tables the new encode route builds"""
    check_decode_fqs(gpu, c1_records(), "c1_10k_s_t4.fqs")


# ---- growth posted from the insert kernel, then recovery --------------------------------------------------------------
def _tiny_tables(monkeypatch):
    monkeypatch.setenv("FQSX_GTAB_INIT", "64")
    monkeypatch.setenv("FQSX_TAB_LOAD_PCT", "85")


def test_growth_posted_by_the_insert_kernel_single_end(monkeypatch):
    _tiny_tables(monkeypatch)
    codec = check_against_fqs(gpu, c1_records(), "c1_10k_s_t4.fqs")
    assert codec.capacity()["growths"] > 0


def test_growth_posted_by_the_insert_kernel_paired_end(monkeypatch):
    """(the pair-table inserts of a phase the insert kernel posts are in already: the recovery must not repeat them)"""
    _tiny_tables(monkeypatch)
    codec = check_against_fqs_pe(gpu, c5_records(), "c5_pe4k_s_t4.fqs")
    assert codec.capacity()["growths"] > 0


# ---- shapes of the offset matrix --------------------------------------------------------------------------------------
def _encode(header, blocks):
    codec = gpu(header)
    return [codec.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)], codec


def test_everything_to_one_owner():
    """400 copies of one read plus poly-A reads, T = 7: one (source, owner) cell holds nearly all entries and most cells are
    empty, so the owners' binary search runs over long runs of equal prefix values."""
    header, blocks, want = _blocks_and_oracle("copies_and_poly_a")
    got, _ = _encode(header, blocks)
    for g in range(len(blocks)):
        assert got[g] == want[g], f"block {g} differs from the oracle"


_t255 = {}


def _t255_blocks_and_oracle():
    if not _t255:
        from fqsqueezer_amd.synth import synth_reads
        from oracle.pyoracle import OracleCodec
        reads = synth_reads(3000, 100, 2000, 29)
        rec = hp.Records([b"@r%d" % i for i in range(len(reads))], reads, reads)
        header = hp.make_header(255, "se_sorted", 1)
        order = np.concatenate(hp.sorted_order(rec))
        # two phases a block while every worker has reads; the last block has fewer reads than workers
        blocks = [hp.block_arrays(rec, order[lo:hi]) for lo, hi in ((0, 1400), (1400, 2800), (2800, 3000))]
        cpu = OracleCodec(header)
        _t255.update(header=header, blocks=blocks, want=[cpu.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)])
    return _t255["header"], _t255["blocks"], _t255["want"]


def test_more_owners_than_lanes_and_empty_sources():
    """T = 255: the owners span four wave rounds of the sender's scan and of the owner's column, most sources push a handful
    of entries, and in the last block most push none."""
    header, blocks, want = _t255_blocks_and_oracle()
    got, _ = _encode(header, blocks)
    for g in range(len(blocks)):
        assert got[g] == want[g], f"block {g} differs from the oracle"


def test_lists_of_many_rounds():
    """T = 1: one source holds thousands of entries a phase -- every wave's slice is many 64-entry rounds long"""
    check_against_fqs(gpu, c1_records(), "c1_10k_s_t1.fqs")


# ---- both paths -------------------------------------------------------------------------------------------------------
def test_sender_and_three_kernel_paths_agree(monkeypatch):
    header, blocks, want = _blocks_and_oracle("genome_2k")

    def run(switch):
        monkeypatch.setenv("FQSX_PART_SENDER", switch)
        codec = gpu(header)
        codec.set_profiling(True)   # (every launch is counted)
        return [codec.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)], codec

    new, c_new = run("1")
    old, c_old = run("0")
    assert new == old == want
    a, b = c_new.capacity(), c_old.capacity()
    assert (a["smers"], a["bmers"], a["growths"]) == (b["smers"], b["bmers"], b["growths"])
    k_new, k_old = c_new.kernel_times(), c_old.kernel_times()
    assert k_new["encode_launches"] == k_old["encode_launches"] > 0
    assert k_old["other_launches"] - k_new["other_launches"] == 2 * k_new["encode_launches"], (k_old, k_new)
