"""Whole files back to FASTQ text (fqsqueezer_amd.fqsread.decompress_fastq / decompress_records): the reference's files against
the digests of what `fqs d` writes for them (tools/make_golden.py --only c24), the files this library writes against their
input, the host fallback for ids beyond the id kernel's staging limits, and the id decoder growing from tiny capacities.
Emulation build and, marked gpu, device 0."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.fqsfile import compress_records, compress_records_pe
from fqsqueezer_amd.fqsread import decompress_fastq, decompress_records
from test_quality_decode import quantised

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
REF_FILES = ["c24_c10_s_i_t4", "c24_c11_pe_o_o_t3", "c24_c11_pe_s_i_t2", "c24_zeros_o_t2", "c24_c10_full_o_t3", "c24_c4_ragged_o_t3"]


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


def _id_lines(text: bytes):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return lines[0:-1:4]


def _check_digests(tag, lib, stats=None):
    d = json.load(open(os.path.join(GOLD, tag + ".json")))
    text = decompress_fastq(open(os.path.join(GOLD, d["fqs"]), "rb").read(), device=0, lib_path=lib, stats=stats)
    assert isinstance(text, tuple) == d["paired"]
    mates = text if d["paired"] else (text,)
    for m, t in enumerate(mates):
        ref = d["mate%d" % (m + 1)]
        ids = _id_lines(t)
        assert len(ids) == ref["reads"], f"{tag}: mate {m + 1}: number of reads"
        assert hashlib.sha256(b"".join(x + b"\n" for x in ids)).hexdigest() == ref["id_lines_sha256"], f"{tag}: mate {m + 1}: id lines differ from `fqs d`"
        assert len(t) == ref["fastq_bytes"] and hashlib.sha256(t).hexdigest() == ref["fastq_sha256"], f"{tag}: mate {m + 1}: FASTQ text differs from `fqs d`"
    return d, mates


# ---- the reference's files -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", REF_FILES)
def test_reference_file_decodes_to_the_text_fqs_d_writes(where, request, tag):
    _check_digests(tag, _lib(where, request))


@pytest.mark.parametrize("where", WHERE)
def test_leading_zeros_are_lost_as_in_the_reference(where, request):
    from fqsqueezer_amd.synth import synth_ids_zeros
    d, (text,) = _check_digests("c24_zeros_o_t2", _lib(where, request))
    got = [x.decode("latin-1") for x in _id_lines(text)]
    assert got == d["id_lines"]
    given = [x.decode("latin-1") for x in synth_ids_zeros(len(got), 24)]
    assert len(given) == len(got) and any(a != b for a, b in zip(given, got)), "the fixture does not exercise the lossy rule"


# ---- the files this library writes -----------------------------------------------------------------------------------------------
def _expected_text(ids, seqs, quals, qmode, imode, thr=20):
    out = []
    for i, s, q in zip(ids, seqs, quals):
        if imode == "instrument":
            i = i[:min(k for k, c in enumerate(i + b" ") if c in b". :")]
        q = np.frombuffer(bytes(q), dtype=np.uint8)
        out.append(i + b"\n" + bytes(s) + b"\n+\n" + quantised(q, qmode, thr).tobytes() + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("qmode,imode", [("lossless", "lossless"), ("illumina_8", "instrument")])
def test_own_single_end_file_comes_back_as_fastq(where, request, order, qmode, imode):
    lib = _lib(where, request)
    rec = c4_records()   # ids "@rag.<n>": no leading zeros, so lossless ids come back as they went in
    data = compress_records(rec, 4, order, 1, lib_path=lib, quality_mode=qmode, id_mode=imode)
    blks = hp.form_blocks(rec, "se_sorted" if order == "s" else "se_original", exact_ties=True)
    idx = np.concatenate(blks)
    want = _expected_text([rec.ids[i] for i in idx], [rec.seq_bytes(int(i)) for i in idx], [rec.qual_bytes(int(i)) for i in idx], qmode, imode)
    st = {}
    assert decompress_fastq(data, device=0, lib_path=lib, stats=st) == want
    assert st["id_host_fallback"] is False


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("qmode,imode", [("lossless", "lossless"), ("illumina_8", "instrument")])
def test_own_paired_file_comes_back_as_fastq(where, request, order, qmode, imode):
    lib = _lib(where, request)
    r1, r2 = (hp.Records(r.ids[:1500], r.seq[:1500], r.qual[:1500]) for r in c5_records())
    data = compress_records_pe(r1, r2, 3, order, 1, lib_path=lib, quality_mode=qmode, id_mode=imode)
    idx = np.concatenate(hp.form_blocks_pe(r1, r2, "pe_sorted" if order == "s" else "pe_original"))
    got = decompress_fastq(data, device=0, lib_path=lib)
    assert isinstance(got, tuple)
    for m, r in enumerate((r1, r2)):
        want = _expected_text([r.ids[i] for i in idx], [r.seq_bytes(int(i)) for i in idx], [r.qual_bytes(int(i)) for i in idx], qmode, imode)
        assert got[m] == want, f"mate {m + 1}"


@pytest.mark.parametrize("where", WHERE)
def test_ids_beyond_the_kernel_limits_come_back_through_the_host_decoder(where, request):
    lib = _lib(where, request)
    rec = c4_records()
    ids = list(rec.ids)
    target = int(hp.form_blocks(rec, "se_sorted", exact_ties=True)[-1][0])   # a read of the last bin
    ids[target] = b"@long." + b"x" * 1500 + b".7"
    rec = hp.Records(ids, rec.seq, rec.qual)
    data = compress_records(rec, 3, "s", 1, lib_path=lib, quality_mode="none", id_mode="lossless")
    blks = hp.form_blocks(rec, "se_sorted", exact_ties=True)
    assert len(blks) > 1 and target not in blks[0]   # the blocks before it are replayed through the host decoder
    st, n = {}, 0
    for idx, (read_len, bases, quals, got, off) in zip(blks, decompress_records(data, device=0, lib_path=lib, stats=st)):
        want, want_off = hp.id_arrays(rec, idx)
        assert np.array_equal(off, want_off) and np.array_equal(got, want), f"block {n}"
        n += 1
    assert n == len(blks) and st["id_host_fallback"] is True


def test_command_line_writes_the_file(built, tmp_path):
    from fqsqueezer_amd import fqsread
    d = json.load(open(os.path.join(GOLD, "c24_c11_pe_o_o_t3.json")))
    o1, o2 = tmp_path / "a.fq", tmp_path / "b.fq"
    assert fqsread.main(["d", os.path.join(GOLD, d["fqs"]), "-out", str(o1), "-out2", str(o2), "-lib", EMU_LIB]) == 0
    assert hashlib.sha256(o1.read_bytes()).hexdigest() == d["mate1"]["fastq_sha256"]
    assert hashlib.sha256(o2.read_bytes()).hexdigest() == d["mate2"]["fastq_sha256"]


def test_decompress_reads_keeps_its_three_tuple(built):
    from fqsqueezer_amd.fqsread import decompress_reads
    first = next(iter(decompress_reads(open(os.path.join(GOLD, "c24_zeros_o_t2.fqs"), "rb").read(), device=0, lib_path=EMU_LIB)))
    assert len(first) == 3


# ---- re-sizing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", ["c24_c10_full_o_t3", "c24_c10_s_i_t4", "c24_c11_pe_o_o_t3", "c24_c11_pe_s_i_t2"])
def test_tiny_initial_capacities_give_the_same_text(where, request, monkeypatch, tag):
    monkeypatch.setenv("FQSX_IDG_INIT", "1")
    st = {}
    _check_digests(tag, _lib(where, request), stats=st)
    assert st["id_host_fallback"] is False and st["id_decoder"]["retries"] >= 1, st
    assert st["id_decoder"]["grow_small"] + st["id_decoder"]["grow_big"] + st["id_decoder"]["grow_out"] >= 1
