"""Reading .fqs files back (fqsqueezer_amd.fqsread.decompress_reads) and the meta decoder it starts from
(fqsx_meta_decode_block): read lengths, bases and qualities of the reference's files and of the files this library writes,
in the order of the file's blocks.  Emulation build and, marked gpu, device 0."""
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records, c10_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.fqsfile import compress_records, compress_records_pe
from test_quality_decode import quantised

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


def _check_file(data, blks, bases_of, quals_of, mode, thr, lib):
    from fqsqueezer_amd.fqsread import decompress_reads
    n = 0
    for idx, (read_len, bases, quals) in zip(blks, decompress_reads(data, device=0, lib_path=lib)):
        want_b, off = bases_of(idx)
        assert np.array_equal(read_len, np.diff(off.astype(np.int64)))
        assert np.array_equal(bases, np.asarray(want_b)), f"block {n}: bases"
        if mode == "none":
            assert len(quals) == int(off[-1]) and (quals == 33 + thr).all()
        else:
            assert np.array_equal(quals, quantised(quals_of(idx)[0], mode, thr)), f"block {n}: qualities"
        n += 1
    assert n == len(blks)


# ---- 4. meta ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("T", [1, 3, 64])
def test_meta_round_trip_all_length_classes(built, T, paired):
    """lengths below 254 (one symbol), 254..65535 (two more bytes) and from 65536 up to the format's 2^24 - 1 (three), several
    blocks through one encoder and one decoder"""
    from fqsqueezer_amd.codec import MetaCodec
    enc, dec = MetaCodec(T, lib_path=EMU_LIB), MetaCodec(T, lib_path=EMU_LIB)
    rng = np.random.default_rng(T)
    edge = np.array([0, 1, 253, 254, 255, 256, 65535, 65536, 65537, (1 << 24) - 1, 100, 100, 150, 151], dtype=np.uint32)
    for b in range(5):
        n = [len(edge), 2, 400, 6, 1000][b]
        lens = np.concatenate([rng.integers(0, 254, n), rng.integers(254, 65536, n), rng.integers(65536, 1 << 24, n), edge]).astype(np.uint32)
        lens = rng.permutation(lens)[:n] if b else edge
        if paired and len(lens) & 1:
            lens = lens[:-1]
        got = dec.decode_block(enc.encode_block(lens, paired), len(lens), paired)
        assert np.array_equal(got, lens), f"block {b}"


def test_meta_stream_that_runs_out_is_refused(built):
    from fqsqueezer_amd.codec import FqsxError, MetaCodec
    lens = np.random.default_rng(2).integers(30, 70000, 600).astype(np.uint32)
    st = MetaCodec(2, lib_path=EMU_LIB).encode_block(lens)
    for bad in ([st[0][:7], st[1]], [st[0], st[1][:len(st[1]) // 2]], [b"", st[1]]):
        with pytest.raises(FqsxError):
            MetaCodec(2, lib_path=EMU_LIB).decode_block(bad, len(lens))


# ---- 5. whole files -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_reads_the_reference_default_mode_file(where, request):
    """c10_full_o_t3.fqs (-qm o -im o): bases and qualities come back, the id stream is skipped"""
    rec = c10_records()
    data = open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()
    _check_file(data, hp.form_blocks(rec, "se_original"), lambda i: hp.block_arrays(rec, i), lambda i: hp.qual_arrays(rec, i), "lossless", 20,
                _lib(where, request))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order,mode", [("o", "lossless"), ("s", "illumina_8"), ("s", "none"), ("s", "lossless")])
def test_reads_own_single_end_files(where, request, order, mode):
    lib = _lib(where, request)
    rec = c4_records()
    data = compress_records(rec, 4, order, 1, lib_path=lib, quality_mode=mode, quality_thr=17)
    blks = hp.form_blocks(rec, "se_sorted" if order == "s" else "se_original", exact_ties=True)
    _check_file(data, blks, lambda i: hp.block_arrays(rec, i), lambda i: hp.qual_arrays(rec, i), mode, 17, lib)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order,mode", [("s", "lossless"), ("o", "illumina_8"), ("o", "none")])
def test_reads_own_paired_files(where, request, order, mode):
    lib = _lib(where, request)
    r1, r2 = (hp.Records(r.ids[:1500], r.seq[:1500], r.qual[:1500]) for r in c5_records())
    data = compress_records_pe(r1, r2, 3, order, 1, lib_path=lib, quality_mode=mode)
    blks = hp.form_blocks_pe(r1, r2, "pe_sorted" if order == "s" else "pe_original")
    _check_file(data, blks, lambda i: hp.block_arrays_pe(r1, r2, i), lambda i: hp.qual_arrays_pe(r1, r2, i), mode, 20, lib)


@pytest.mark.parametrize("where", WHERE)
def test_reads_the_reference_paired_file(where, request):
    import json
    d = json.load(open(os.path.join(GOLD, "c23_c5_pe_qo_t3.json")))
    r1, r2 = (hp.Records(r.ids[:d["pairs"]], r.seq[:d["pairs"]], r.qual[:d["pairs"]]) for r in c5_records())
    data = open(os.path.join(GOLD, "c23_c5_pe_qo_t3.fqs"), "rb").read()
    _check_file(data, hp.form_blocks_pe(r1, r2, "pe_sorted"), lambda i: hp.block_arrays_pe(r1, r2, i), lambda i: hp.qual_arrays_pe(r1, r2, i),
                "lossless", 20, _lib(where, request))
