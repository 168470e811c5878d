"""Complete .fqs files written around the DNA path: byte identity with the reference's own files and
round trip through the unmodified reference decompressor (oracle/_ref/fqs-1.1 d; its verdict on the files is also kept as
data in tests/golden/c4_ragged_ref_decode.json, so that the round trip is checked where the binary is not built)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import json

from conftest import EMU_LIB, GOLD, IM, QM, ROOT, c1_records, c4_records, c10_records, c11_records, check_full_file_digest, digest_records, pe_digest_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.fqsfile import compress_records, compress_records_pe

REF = os.path.join(ROOT, "oracle", "_ref", "fqs-1.1")


def _decode_with_reference(data: bytes, tmp_path):
    f = tmp_path / "x.fqs"
    f.write_bytes(data)
    out = tmp_path / "x.fq"
    subprocess.check_call([REF, "d", "-out", str(out), str(f)], stdout=subprocess.DEVNULL)
    return out.read_bytes().split(b"\n")[1::4]


def _check_reference_decodes(data: bytes, rec, order: str, T: int, tmp_path):
    """The reference decoder reads `data` back into the reads of `rec`: `data` is byte for byte the file the reference wrote for
    them and decoded with `fqs-1.1 d` (tools/make_golden.py c4), and the read lines it decoded are `rec`'s, in the file's order.
    Where oracle/_ref/fqs-1.1 is built, it decodes `data` here as well."""
    g = json.load(open(os.path.join(GOLD, "c4_ragged_ref_decode.json")))[f"{order}_t{T}"]
    order_idx = range(len(rec)) if order == "o" else np.concatenate(hp.sorted_order(rec))
    want = [rec.seq[int(i)] for i in order_idx]
    assert len(data) == g["file_bytes"] and hashlib.sha256(data).hexdigest() == g["file_sha256"], "not the file the reference decoded"
    assert len(want) == g["decoded_reads"]
    assert hashlib.sha256(b"".join(x + b"\n" for x in want)).hexdigest() == g["decoded_sha256"], "the reference decoded other reads"
    if os.path.exists(REF):
        assert _decode_with_reference(data, tmp_path)[:len(want)] == want


def _lib(request):
    return None if request.node.get_closest_marker("gpu") else EMU_LIB


@pytest.mark.parametrize("name,rec_fn,T,gs", [("c4_ragged_o_t3.fqs", c4_records, 3, 1), ("c1_10k_o_t4.fqs", c1_records, 4, 1)])
def test_file_identical_to_reference_original_order(built, name, rec_fn, T, gs):
    data = compress_records(rec_fn(), T, "o", gs, lib_path=EMU_LIB)
    assert data == open(os.path.join(GOLD, name), "rb").read()


def test_default_mode_file_identical_to_reference(built):
    """-qm o -im o: ids, qualities, read lengths and DNA -- the whole file byte for byte."""
    data = compress_records(c10_records(), 3, "o", 1, lib_path=EMU_LIB, quality_mode="lossless", id_mode="lossless")
    assert data == open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()


FULL_SE = [("c10_full_s_i8_t4.json", "s", "8", "i", 4), ("c10_full_s_oo_t2.json", "s", "o", "o", 2), ("c10_full_o_i2_t5.json", "o", "2", "i", 5)]
FULL_PE = [("c11_pe_full_s_o4_t3.json", "s", "4", "o", 3), ("c11_pe_full_o_io_t2.json", "o", "o", "i", 2)]


@pytest.mark.parametrize("name,om,qm,im,T", FULL_SE)
def test_full_mode_files_match_reference_digests(built, name, om, qm, im, T):
    check_full_file_digest(compress_records(c10_records(), T, om, 1, lib_path=EMU_LIB, quality_mode=QM[qm], id_mode=IM[im]), name)


@pytest.mark.parametrize("name,om,qm,im,T", FULL_PE)
def test_full_mode_paired_files_match_reference_digests(built, name, om, qm, im, T):
    r1, r2 = c11_records()
    check_full_file_digest(compress_records_pe(r1, r2, T, om, 1, lib_path=EMU_LIB, quality_mode=QM[qm], id_mode=IM[im]), name)


@pytest.mark.parametrize("order", ["o", "s"])
def test_reference_decoder_reads_our_file(built, tmp_path, order):
    rec = c4_records()
    _check_reference_decodes(compress_records(rec, 5, order, 1, lib_path=EMU_LIB), rec, order, 5, tmp_path)


@pytest.mark.gpu
def test_gpu_full_mode_files_identical_to_reference():
    data = compress_records(c10_records(), 3, "o", 1, quality_mode="lossless", id_mode="lossless")
    assert data == open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()
    name, om, qm, im, T = FULL_SE[0]
    check_full_file_digest(compress_records(c10_records(), T, om, 1, quality_mode=QM[qm], id_mode=IM[im]), name)
    name, om, qm, im, T = FULL_PE[0]
    r1, r2 = c11_records()
    check_full_file_digest(compress_records_pe(r1, r2, T, om, 1, quality_mode=QM[qm], id_mode=IM[im]), name)


@pytest.mark.gpu
def test_gpu_file_identical_to_reference_and_decodes(tmp_path):
    data = compress_records(c1_records(), 4, "o", 1)
    assert data == open(os.path.join(GOLD, "c1_10k_o_t4.fqs"), "rb").read()
    rec = c4_records()
    _check_reference_decodes(compress_records(rec, 64, "s", 1), rec, "s", 64, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c14_pe150_s_q8_t8.json", "c15_pe150_s_oo_t4.json"])
def test_gpu_paired_end_150bp_files_match_reference(name):
    """BASELINE configs[2]'s shape (150 bp pairs, -om s -qm 8; 100 k pairs, T = 8) and configs[4]'s modes (-qm o -im o):
    every stream of every block, then the whole file, against the reference's own file."""
    d = json.load(open(os.path.join(GOLD, name)))
    r1, r2 = pe_digest_records(d)
    check_full_file_digest(compress_records_pe(r1, r2, d["threads"], d["om"], d["gs"], quality_mode=QM[d["qm"]], id_mode=IM[d["im"]]), name)


@pytest.mark.gpu
def test_gpu_sorted_order_of_1M_reads_is_the_reference_order():
    """N3 against the reference itself: the GPU sort pre-pass orders the metric's 1 M x 150 bp file; the id stream (which
    sees the order of equal reads too) and the DNA stream of the resulting file match the reference's `-om s -im o` file."""
    name = "c16_1M150_s_ids_t8.json"
    d = json.load(open(os.path.join(GOLD, name)))
    check_full_file_digest(compress_records(digest_records(d), d["threads"], "s", d["gs"], quality_mode="none", id_mode="lossless"), name)


# ---- far fewer reads than workers: 40 reads / pairs and one read / pair at -t 64 (tools/make_golden.py c27) -------------------------
def _check_tiny_file(tag, lib_path):
    """compress_records* writes the reference's file byte for byte -- every stream of the 64 workers, most of which have no
    read -- and fqsread decodes that file to the input text"""
    from fqsqueezer_amd.fqsread import decompress_fastq
    from fqsqueezer_amd.synth import C27_FILES, fastq_text, synth_c27
    inputs = [synth_c27(n) for n in C27_FILES[tag]]
    recs = [hp.Records(*x) for x in inputs]
    want = open(os.path.join(GOLD, tag + ".fqs"), "rb").read()
    header, blocks = hp.parse_fqs(want)
    assert header[4] == 64 and sum(b.n_reads for b in blocks) == len(recs) * len(recs[0]) < 2 * 64
    compress = compress_records_pe if len(recs) == 2 else compress_records
    data = compress(*recs, 64, "o", 1, lib_path=lib_path, quality_mode="lossless", id_mode="lossless")
    assert data == want
    text = decompress_fastq(want, lib_path=lib_path)
    assert (list(text) if len(recs) == 2 else [text]) == [fastq_text(*x) for x in inputs]


TINY_FILES = ["c27_tiny_se_o_oo_t64", "c27_tiny_pe_o_oo_t64", "c27_one_se_o_oo_t64", "c27_one_pe_o_oo_t64"]


@pytest.mark.parametrize("tag", TINY_FILES)
def test_files_with_fewer_reads_than_workers_identical_to_reference(built, tag):
    _check_tiny_file(tag, EMU_LIB)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TINY_FILES)
def test_gpu_files_with_fewer_reads_than_workers_identical_to_reference(tag):
    _check_tiny_file(tag, None)
