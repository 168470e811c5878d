"""FASTQ text to a .fqs file (fqsfile.compress_fastq, `python -m fqsqueezer_amd.fqsfile e`): the same bytes as compress_records*
on read_fastq of the text, the reference's own files (the fixtures tests/test_fqs_file.py pins compress_records to, and c25:
`+id` separator lines and a last record without its line feed, tools/make_golden.py --only c25), the two refusals, the host
id coder for ids beyond the kernel's limits, and the command line.  Emulation build and, marked gpu, device 0."""
import functools
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records, c10_records, c11_records, check_full_file_digest
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.fqsfile import compress_fastq, compress_records, compress_records_pe
from fqsqueezer_amd.fqsread import decompress_fastq
from fqsqueezer_amd.synth import fastq_text, synth_c25_text

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
MODES = [pytest.param("lossless", "lossless", id="qm_o-im_o"), pytest.param("illumina_8", "instrument", id="qm_8-im_i")]


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


def _text(rec):
    return fastq_text(rec.ids, [rec.seq_bytes(i) for i in range(len(rec))], [rec.qual_bytes(i) for i in range(len(rec))])


@functools.lru_cache(maxsize=None)
def texts(name: str):
    """FASTQ text of a fixture's records: bytes, or (mate 1, mate 2)"""
    rec = {"c4": c4_records, "c10": c10_records, "c11": c11_records, "c5": c5_records}[name]()
    return tuple(_text(r) for r in rec) if isinstance(rec, tuple) else _text(rec)


def _records(tmp_path, text, tag="x"):
    f = tmp_path / (tag + ".fq")
    f.write_bytes(text)
    return hp.read_fastq(str(f))


# ---- the same bytes as the Records path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("name", ["c4", "c10"])
def test_single_end_file_equals_compress_records(where, request, tmp_path, name, order, qm, im):
    lib = _lib(where, request)
    want = compress_records(_records(tmp_path, texts(name)), 3, order, 1, lib_path=lib, quality_mode=qm, id_mode=im)
    assert compress_fastq(texts(name), threads=3, order=order, genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib) == want


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("qm,im", MODES)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("name", ["c11", "c5"])
def test_paired_file_equals_compress_records_pe(where, request, tmp_path, name, order, qm, im):
    lib = _lib(where, request)
    t1, t2 = texts(name)
    want = compress_records_pe(_records(tmp_path, t1, "a"), _records(tmp_path, t2, "b"), 2, order, 1, lib_path=lib, quality_mode=qm, id_mode=im)
    assert compress_fastq(t1, t2, threads=2, order=order, genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=lib) == want


# ---- the reference's own files ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_single_end_original_order_file_is_the_reference_file(where, request):
    data = compress_fastq(texts("c10"), threads=3, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=_lib(where, request))
    assert data == open(os.path.join(GOLD, "c10_full_o_t3.fqs"), "rb").read()


@pytest.mark.parametrize("where", WHERE)
def test_single_end_sorted_file_matches_the_reference_digest(where, request):
    data = compress_fastq(texts("c10"), threads=2, order="s", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=_lib(where, request))
    check_full_file_digest(data, "c10_full_s_oo_t2.json")


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,order,qm,im,T", [("c11_pe_full_s_o4_t3.json", "s", "illumina_4", "lossless", 3), ("c11_pe_full_o_io_t2.json", "o", "lossless", "instrument", 2)])
def test_paired_file_matches_the_reference_digest(where, request, name, order, qm, im, T):
    t1, t2 = texts("c11")
    check_full_file_digest(compress_fastq(t1, t2, threads=T, order=order, genome_size_mbp=1, quality_mode=qm, id_mode=im, lib_path=_lib(where, request)), name)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order", ["o", "s"])
def test_ragged_file_is_the_reference_file(where, request, order):
    data = compress_fastq(texts("c4"), threads=3, order=order, genome_size_mbp=1, quality_mode="none", id_mode="none", lib_path=_lib(where, request))
    assert data == open(os.path.join(GOLD, "c4_ragged_%s_t3.fqs" % order), "rb").read()


@pytest.mark.parametrize("where", WHERE)
def test_c25_unterminated_last_record_and_plus_id_lines_as_the_reference(where, request):
    """The reference drops the last record when its quality line lacks the line feed (1999 of the 2000 reads are in its file),
    and the `+id` separator lines count towards the block boundaries and the workers' offsets."""
    lib = _lib(where, request)
    text = synth_c25_text()
    assert not text.endswith(b"\n") and text.count(b"\n") == 4 * 2000 - 1
    st = {}
    data = compress_fastq(text, threads=3, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib, stats=st)
    assert data == open(os.path.join(GOLD, "c25_plus_nolf_o_t3.fqs"), "rb").read()
    assert st["parse"][0]["tail_bytes"] > 0 and sum(b.n_reads for b in hp.parse_fqs(data)[1]) == 1999
    check_full_file_digest(compress_fastq(text, threads=2, order="s", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib),
                           "c25_plus_nolf_s_t2.json")


# ---- refusals, the id coder's limits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_quality_length_mismatch_is_refused(where, request):
    text = texts("c4")[:20000]
    text = text[:text.rindex(b"\n@")] + b"\n@bad\nACGT\n+\n!!!\n"
    with pytest.raises(ValueError, match="quality line"):
        compress_fastq(text, threads=2, order="o", genome_size_mbp=1, lib_path=_lib(where, request))


@pytest.mark.parametrize("where", WHERE)
def test_mate_files_of_different_lengths_are_refused(where, request):
    t1, t2 = texts("c11")
    with pytest.raises(ValueError, match="different numbers of records"):
        compress_fastq(t1[:30000], t2[:20000], threads=2, order="o", genome_size_mbp=1, lib_path=_lib(where, request))


@pytest.mark.parametrize("where", WHERE)
def test_an_id_beyond_the_kernel_limits_goes_to_the_host_id_coder(where, request):
    lib = _lib(where, request)
    rec = c4_records()
    ids = list(rec.ids[:600])
    ids[411] = b"@long." + b"x" * 1092 + b".7"   # an id line of 1100 bytes; no leading zeros anywhere, so lossless ids come back as given
    assert len(ids[411]) == 1100
    text = fastq_text(ids, rec.seq[:600], rec.qual[:600])
    st = {}
    data = compress_fastq(text, threads=2, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib, stats=st)
    assert st["gpu_ids"] is False and st["parse"][0]["max_id_line"] == 1101
    assert decompress_fastq(data, device=0, lib_path=lib) == text
    st = {}
    compress_fastq(texts("c4")[:50000], threads=2, order="o", genome_size_mbp=1, quality_mode="none", id_mode="lossless", lib_path=lib, stats=st)
    assert st["gpu_ids"] is True


# ---- command line -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_command_line_e_then_d_round_trips(where, request, tmp_path):
    from fqsqueezer_amd import fqsfile, fqsread
    lib = _lib(where, request)
    extra = ["-lib", lib] if lib else []
    se = texts("c4")[:texts("c4").index(b"\n@rag.801\n") + 1]   # ids "@rag.<n>": no leading zeros
    t1, t2 = (t[:t.index(b"\n", 150000) + 1] for t in texts("c5"))
    t1, t2 = (t[:t.rindex(b"\n@", 0, len(t) - 1) + 1] for t in (t1, t2))
    i1, i2, i3 = tmp_path / "se.fq", tmp_path / "m1.fq", tmp_path / "m2.fq"
    for f, t in ((i1, se), (i2, t1), (i3, t2)):
        f.write_bytes(t)
    common = ["-t", "2", "-gs", "1", "-om", "o", "-qm", "o", "-im", "o"]
    out = tmp_path / "se.fqs"
    assert fqsfile.main(["e", "-s"] + common + ["-out", str(out), str(i1)] + extra) == 0
    assert out.read_bytes() == compress_fastq(se, threads=2, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib)
    back = tmp_path / "se_back.fq"
    assert fqsread.main(["d", str(out), "-out", str(back)] + extra) == 0
    assert back.read_bytes() == se
    out = tmp_path / "pe.fqs"
    assert fqsfile.main(["e", "-p"] + common + ["-out", str(out), str(i2), str(i3)] + extra) == 0
    assert out.read_bytes() == compress_fastq(t1, t2, threads=2, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib)
    b1, b2 = tmp_path / "b1.fq", tmp_path / "b2.fq"
    assert fqsread.main(["d", str(out), "-out", str(b1), "-out2", str(b2)] + extra) == 0
    assert b1.read_bytes() == t1 and b2.read_bytes() == t2
