"""DNA-stream decoder (csrc/fqsx_dec.h, kernels k_decode_{se,pe}_{orig,sorted}) pinned from the sides the encoder is pinned from:
tiny tables and their overflow chains, chunked tables, growth in mid-block, T up to 255, saturated counters, corrections followed by
duplicates, reads shorter than the k-mers and longer than the LDS staging, blocks with fewer reads than workers.

Every case sends a sequence of blocks through ONE encoder and ONE decoder (_round_trip): each block must come back byte for byte -- the
reference for "right bases" is the input itself -- and after each block the decoder's tables must hold exactly what the encoder's
hold (a decoder that returns the right bases but learns something else fails blocks later; the comparison pins it to the block
where it happens).  Where the reference's own file or digest of the input exists, the encoder's streams are compared with it first,
so that the bytes being decoded are known to be the reference's.  Every case runs on the emulation build (a 1-lane wave) and,
marked gpu, on device 0."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c1_records, c4_records, c5_records, c7_records, c20_records, digest_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.synth import synth_pairs, synth_reads, synth_two_haplotypes

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
MODES = ["se_original", "se_sorted", "pe_original", "pe_sorted"]
# what the decoder must have learnt exactly as the encoder did (fqsx_dna_capacity): all five are results of the same insert phases
# over the same k-mers, pairs and contexts in both directions, so none is dropped
KEYS = ("smers", "bmers", "pairs", "contexts", "growths")


def _codec(where, request, **kw):
    from fqsqueezer_amd.codec import DnaCodec
    if where == "emu":
        request.getfixturevalue("built")
        return lambda h: DnaCodec(h, lib_path=EMU_LIB, **kw)
    return lambda h: DnaCodec(h, device=0, **kw)


def _round_trip(mk, header, blocks, want=None):
    """blocks of (bases, off) through ONE encoder and ONE decoder.  want[g] (optional): the reference's streams of block g -- a list
    of the T streams, or the {"bytes", "sha256"} entry of a digest fixture.  Returns (enc, dec)."""
    enc, dec = mk(header), mk(header)
    for g, (bases, off) in enumerate(blocks):
        streams = enc.encode_block(bases, off, g)
        if want is not None:
            if isinstance(want[g], dict):
                h = hashlib.sha256()
                for s in streams:
                    h.update(s)
                assert (sum(len(s) for s in streams), h.hexdigest()) == (want[g]["bytes"], want[g]["sha256"]), f"block {g}: not the reference's streams"
            else:
                assert streams == want[g], f"block {g}: not the reference's streams"
        out = dec.decode_block(streams, off, g)
        assert np.array_equal(out, np.asarray(bases)), f"block {g} decoded wrongly"
        ce, cd = enc.capacity(), dec.capacity()
        assert {k: cd[k] for k in KEYS} == {k: ce[k] for k in KEYS}, f"block {g}: the decoder's tables differ from the encoder's"
    return enc, dec


def _rec(reads):
    return hp.Records([b"@r%d" % i for i in range(len(reads))], reads, reads)


def _order(rec, mode):
    """read (pair) indices in the order the mode codes them"""
    r1 = rec[0] if mode.startswith("pe") else rec
    return np.concatenate(hp.sorted_order(r1)) if mode.endswith("sorted") else np.arange(len(r1))


def _arrays(rec, mode, idx):
    return hp.block_arrays_pe(rec[0], rec[1], idx) if mode.startswith("pe") else hp.block_arrays(rec, idx)


def _cut(rec, mode, sizes, rest=False):
    """consecutive blocks of the given numbers of reads (pairs: mates stay together), then, if asked for, the rest in one block"""
    order, blocks, lo = _order(rec, mode), [], 0
    for n in list(sizes) + ([len(order)] if rest else []):
        if lo < len(order):
            blocks.append(_arrays(rec, mode, order[lo:lo + n]))
        lo += n
    return blocks


def _fqs_blocks(rec, name):
    """header, blocks and the reference's DNA streams of a reference file of `rec`"""
    header, ref = hp.parse_fqs(open(os.path.join(GOLD, name), "rb").read())
    mode = MODES[header[5]]
    blks = hp.form_blocks_pe(rec[0], rec[1], mode) if header[5] >= 2 else hp.form_blocks(rec, mode)
    assert len(blks) == len(ref)
    want = [[b.streams[w][hp.STREAM_DNA] for w in range(header[4])] for b in ref]
    return header, [_arrays(rec, mode, idx) for idx in blks], want


def _tables(monkeypatch, kind):
    """environment of a table kind; returns the DnaCodec arguments that go with it"""
    if kind == "tiny":            # 64-slot sub-tables driven to 85 % load: overflow chains, dozens of growths
        monkeypatch.setenv("FQSX_GTAB_INIT", "64")
        monkeypatch.setenv("FQSX_TAB_LOAD_PCT", "85")
        monkeypatch.setenv("FQSX_TAB_AFTER_PCT", "80")
    elif kind == "chunked":       # one chunk per sub-table, grown sub-table by sub-table (from 256 slots, so that they do grow)
        monkeypatch.setenv("FQSX_GTAB_INIT", "256")
        monkeypatch.setenv("FQSX_CHUNK_STEP_KB", "1")
        return {"chunked_tables": True}
    else:
        assert kind == "default"
    return {}


# ---- a. the look-up requested a position ahead, after a revert ----------------------------------------------------------------
# (reads or pairs, seed) per mode: inputs on which the decoder that compared bucket a alone decodes block 1 wrongly on the emulation build
STALE = {"se_original": (5000, 2), "se_sorted": (5000, 1), "pe_original": (3000, 4), "pe_sorted": (3000, 1)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", WHERE)
def test_stale_prefetch_after_a_revert(where, mode, request, monkeypatch):
    """suffix_dec requests the two buckets of position i + 1's b-mer before position i's LV_BMER_UNC revert can replace the k-mer.  With
    two-choice buckets the new k-mer can share bucket a with the old one and have another bucket b: a decoder that reuses the request
    on `a` alone counts siblings out of the old k-mer's bucket b and chain, sees other counts than the encoder and decodes other bases
    with no error (first item).  Tables of 64 slots per owner at T = 255 keep the sub-tables at a few hundred buckets
    (b-mer slots / 255 / 4 = 440-630 here), 50 x (150 bp) coverage of 3 kbp with 2 % substitutions makes reverts frequent.
    Measured on the emulation build with the comparison on `a` alone: block 1 of each of the four inputs "decoded wrongly" or ends in
    a decode error; with a and b compared all pass and dec_refetch = 1535 / 1468 / 1795 / 1851 (se_o / se_s / pe_o / pe_s).  The
    GPU runs four times the reads in four times the blocks."""
    monkeypatch.setenv("FQSX_GTAB_INIT", "64")
    n, seed = STALE[mode]
    k = 4 if where == "gpu" else 1
    if mode.startswith("pe"):
        r1, r2 = synth_pairs(k * n, 150, 3000, seed, frag_min=200, frag_max=400, sub_rate=0.02)
        rec = (_rec(r1), _rec(r2))
    else:
        rec = _rec(synth_reads(k * n, 150, 3000, seed, sub_rate=0.02))
    blocks = [_arrays(rec, mode, idx) for idx in np.array_split(_order(rec, mode), 2 * k)]
    enc, dec = _round_trip(_codec(where, request), hp.make_header(255, mode, 1), blocks)
    # the case reaches the branch: requests made a position ahead were dropped and the buckets looked up again -- at least a third
    # of the smallest count measured (1468); the GPU's input holds four times the reads
    assert dec.stats()["dec_refetch"] >= 480 and enc.stats()["dec_refetch"] == 0, dec.stats()
    assert enc.capacity()["growths"] >= 2


# ---- b. modes x workers x table kinds on inputs with edges -----------------------------------------------------------------------
WORKERS = [1, 3, 64, 255]
KINDS = ["default", "tiny", "chunked"]
# GPU: the product.  Emulation build: every mode at every T once, and (the kinds rotate with mode and T) every kind in every mode.
MATRIX = [pytest.param("gpu", m, t, k, id=f"gpu-{m}-t{t}-{k}", marks=pytest.mark.gpu) for m in MODES for t in WORKERS for k in KINDS] + \
         [pytest.param("emu", m, t, KINDS[(i + j) % 3], id=f"emu-{m}-t{t}-{KINDS[(i + j) % 3]}") for i, m in enumerate(MODES) for j, t in enumerate(WORKERS)]


@pytest.mark.parametrize("where,mode,T,kind", MATRIX)
def test_round_trip_matrix(where, mode, T, kind, request, monkeypatch):
    """single-end: c4 (ragged, N runs, duplicates, reads shorter than the k-mers) and c7 (20-31 bp and 4200-6000 bp reads: shorter than
    the b-mer, longer than the LDS staging); paired: c5 and c20 (5000 bp mates).  Blocks of 700, 31, 2 and 1 reads (pairs): fewer reads
    than workers, a single read, a single pair; on the GPU the rest of the input follows as one more block."""
    mk = _codec(where, request, **_tables(monkeypatch, kind))
    header = hp.make_header(T, mode, 1)
    gpu = where == "gpu"
    if mode.startswith("pe"):
        cases = [(c5_records(), [700, 31, 2, 1]), (c20_records(), [40, 2, 1])]
    else:
        cases = [(c4_records(), [700, 31, 2, 1]), (c7_records(), [700, 31, 2, 1])]
    for rec, sizes in cases:
        enc, dec = _round_trip(mk, header, _cut(rec, mode, sizes, rest=gpu))
        # the tiny and the chunked tables did grow (the chunked re-insert, the chains' re-insert were seen by the decoder).  Measured
        # on the emulation build over all modes and both inputs, blocks without the rest: tiny 18-74 / 8-62 / 2-12 / 2 growths at
        # T = 1 / 3 / 64 / 255, chunked 4-14 / 2-12 / 2-4 / 2; the floors are the smallest of them (the GPU codes more: no fewer)
        if kind != "default":
            assert dec.capacity()["growths"] >= (8 if kind == "tiny" and T <= 3 else 2), dec.capacity()


# ---- c. saturated counters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["se_original", "se_sorted"])
@pytest.mark.parametrize("where", WHERE)
def test_saturated_counters(where, mode, request):
    """60 000 x 100 bp over two haplotypes of 300 bp that differ every 40 bases (10 000 x per allele): both alleles of a site at the
    counter maximum (LV_MIXED), the LV_BMER_UNC revert and the probabilistic counters above their thresholds are walked by the decoder.
    (At this number of reads a 2 kbp genome does not get there: the oracle counts mixed = 0 in both modes.)  That the input reaches
    them is asserted on the oracle, as for the c13 fixture (tests/test_oracle_golden.py), whose streams the encoder's must equal; the
    floors are a tenth or less of what the oracle counts on this input (sorted mode, the smaller: mixed 5842, bmer_unc 8, draws_b
    1.2 M, draws_s 1.0 M)."""
    from oracle.pyoracle import OracleCodec
    rec = _rec(synth_two_haplotypes(60000, 100, 300, 13, snp_every=40))
    header = hp.make_header(4, mode, 1)
    blocks = [_arrays(rec, mode, idx) for idx in np.array_split(_order(rec, mode), 3)]
    oc = OracleCodec(header)
    want = [oc.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)]
    lv = oc.levels()
    assert lv["mixed"] > 500 and lv["bmer_unc"] > 0 and lv["draws_b"] > 100_000 and lv["draws_s"] > 100_000, lv
    _round_trip(_codec(where, request), header, blocks, want)


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("om", ["o", "s"])
def test_saturated_counters_c13_gpu(om, request):
    """the slow extra of test_saturated_counters[gpu-*]: the c13 inputs themselves (300 000 x 100 bp, ~12 000 x coverage, 30 Mbases
    through the four waves of the fixture's T = 4): the encoder's streams are the reference's (digest), and every block decodes"""
    d = json.load(open(os.path.join(GOLD, f"c13_sat_{om}_t4.json")))
    rec, header = digest_records(d), bytes.fromhex(d["header"])
    mode = MODES[header[5]]
    blks = hp.form_blocks(rec, mode)
    assert len(blks) == d["n_blocks"]
    _round_trip(_codec("gpu", request), header, [_arrays(rec, mode, idx) for idx in blks], d["blocks"])


# ---- d. corrections, then duplicates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 64])
@pytest.mark.parametrize("where", WHERE)
def test_long_reads_with_corrections_followed_by_duplicates(where, T, request):
    """350 bp reads with substitutions, each three times, sorted mode: what test_hip_long_reads_with_corrections_followed_by_duplicates
    encodes (there 2500 reads x 3 against the oracle; the emulation build takes 500 x 3) is decoded"""
    base = synth_reads(2500 if where == "gpu" else 500, 350, 60000, 41, sub_rate=0.01)
    reads = np.repeat(base, 3, axis=0)
    rec = _rec(reads[np.random.Generator(np.random.PCG64(5)).permutation(len(reads))])
    order = _order(rec, "se_sorted")
    B = 1200 if where == "gpu" else 400
    blocks = [hp.block_arrays(rec, order[lo:lo + B]) for lo in range(0, len(order) - 2 * T, B)]
    _round_trip(_codec(where, request), hp.make_header(T, "se_sorted", 1), blocks)


# ---- e. growth posted in mid-block, decode side ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_10k_s_t4.fqs", "c1_10k_o_t4.fqs", "c5_pe4k_o_t4.fqs", "c5_pe4k_s_t4.fqs"])
@pytest.mark.parametrize("where", WHERE)
def test_growth_posted_by_the_device_decode_side(where, name, request, monkeypatch):
    """Tables that start at 256 slots per owner (pair table: 64) grow in most blocks: the decoder's phases are stopped, grown and taken
    up again like the encoder's.  Streams are the reference's files'; the decoder's growths equal the encoder's (_round_trip) and reach
    the floors of the encoder's tests of the same set-up (>= 4: test_chunked_tables_grow_sub_table_by_sub_table, same input and
    tables; paired >= 8 and a grown pair table: test_emu_paired_end_growth_posted_by_the_device_is_recovered)."""
    monkeypatch.setenv("FQSX_GTAB_INIT", "256")
    paired = name.startswith("c5")
    if paired:
        monkeypatch.setenv("FQSX_PTAB_INIT", "64")
    header, blocks, want = _fqs_blocks(c5_records() if paired else c1_records(), name)
    enc, dec = _round_trip(_codec(where, request), header, blocks, want)
    cap = dec.capacity()
    if paired:
        assert cap["growths"] >= 8 and cap["pair_slots"] > 64 * 4 and cap["pair_slots"] == enc.capacity()["pair_slots"], cap
    else:
        assert cap["growths"] >= 4, cap


# ---- f. anchor positions of three bytes ----------------------------------------------------------------------------------------------
_FAR = {}


def _far_anchor_case(mode):
    """(header, blocks, the oracle's streams, the oracle's branch counters) of the input of test_anchor_positions_of_three_bytes,
    computed once per mode for the emulation build and the GPU"""
    if mode not in _FAR:
        from oracle.pyoracle import OracleCodec
        rng = np.random.Generator(np.random.PCG64(65536))
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        mate1, tail = acgt[rng.integers(0, 4, 300)], acgt[rng.integers(0, 4, 34000)]
        blocks = []
        for _ in range(2):
            reads = [r for _ in range(4) for r in (mate1, np.concatenate([acgt[rng.integers(0, 4, 66000)], tail]))]
            off = np.zeros(len(reads) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(r) for r in reads])
            blocks.append((np.concatenate(reads), off))
        header = hp.make_header(2, mode, 1)
        oc = OracleCodec(header)
        want = [oc.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)]
        _FAR[mode] = (header, blocks, want, oc.levels())
    return _FAR[mode]


@pytest.mark.parametrize("mode", ["pe_original", "pe_sorted"])
@pytest.mark.parametrize("where", WHERE)
def test_anchor_positions_of_three_bytes(where, mode, request):
    """The anchor position of a second mate is coded in one symbol, in three (the 254 escape: positions up to 65535; c20 reaches
    it, tests/test_oracle_golden.py) or in four (the 255 escape, MPOS_ENC / MPOS_DEC classes 3-5: positions from 65536, in mates
    of up to 2^24 - 1 bases).  8 pairs in two blocks of 4, T = 2: every first mate is the same 300 random bases, every second
    mate 66 000 fresh random bases and one shared random tail of 34 000.  The minimizer windows of the last third of a 100 000-base
    mate start at about 66 660, so the only minimizers of a second mate that the pair table can offer a later pair lie in the
    shared tail, above 65 536.  That the four-symbol branch is reached is counted by the oracle (anchor_4); the encoder under
    test writes the oracle's streams byte for byte, so it coded the same escapes, and the decoder that returns the input decoded
    them.  Measured: a parametrisation takes 13.9 s (pe_original) / 12.8 s (pe_sorted) on the emulation build and 6.9 s / 5.4 s on
    the MI355X, of which 2.1 s are the oracle's (once per mode).  Blocks of 3 pairs instead of 4 were tried and are no answer: 6.6 s /
    5.1 s on the GPU, 12.3 s / 11.9 s on the emulation build -- the time is the codecs' (tables of the full default size, made and
    compared three times) more than the bases' -- so the input stays the 8 pairs."""
    header, blocks, want, lv = _far_anchor_case(mode)
    assert lv["anchor_4"] > 0, lv
    _round_trip(_codec(where, request), header, blocks, want)


# ---- g. empty reads at a worker's start -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["se_original", "pe_original", "pe_sorted"])
@pytest.mark.parametrize("where", WHERE)
def test_empty_first_read_of_a_worker(where, mode, request):
    """T = 2, blocks of four reads (two pairs): an empty read in front of three of 100 bases, an empty read at the start of either
    worker, four empty reads, and once more the second block (an empty read whose predecessor is empty too is a duplicate).  The
    encoder never sets the duplicate flag for a worker's first read (read_head: no previous read), so an empty first read is
    coded in full, and the decoder must take it so; where a worker has a previous read, an empty read after an empty one is
    coded by the flag.  In the original-order modes reads of 3 bases, shorter than every prefix, end the last block: their
    prefix is not written past them.
    Not covered: se_sorted, and reads shorter than the p-mer in pe_sorted.  There the encoder builds the p-mer of the sorted
    prefix from positions beyond the read (rd_sym), and the blocks above do not come back (se_sorted: blocks 0, 1 and 3 decode
    to other bases; the 3-base reads end in device error 8 in both sorted modes) -- before the decoder's checks on damaged
    streams as after them, measured on the emulation build of either state.
    On the MI355X block 1 (the empty first read of worker 1) came back wrong in se_original before read_head padded the staged
    code line: for a read shorter than the prefix rd_sym took the missing positions from LDS that the read had not staged, and a
    byte above 4 there is no symbol of the letter models."""
    r = synth_reads(4, 100, 5000, 17)
    e, s = np.zeros(0, dtype=np.uint8), r[3][:3]
    cases = [[e, r[0], r[1], r[2]], [e, r[0], e, r[1]], [e, e, e, e], [e, r[0], e, r[1]]]
    if mode.endswith("original"):
        cases.append([r[2], s, r[3], s])
    blocks = []
    for reads in cases:
        off = np.zeros(5, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in reads])
        blocks.append((np.concatenate(reads), off))
    _round_trip(_codec(where, request), hp.make_header(2, mode, 1), blocks)
