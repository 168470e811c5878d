"""Whole files streamed back to FASTQ text (fqsqueezer_amd.fqsread.decompress_fastq_chunks): one chunk per container block, the
columns left on the device and the text assembled there (codec.FastqText), against the digests of what the reference's
`fqs d` writes, against decompress_fastq, and the file read piece by piece (hostpipe.iter_fqs).  Emulation build and, marked
gpu, device 0."""
import hashlib
import io
import json
import os

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, c4_records, c5_records
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DeviceColumns, DnaCodec, IdCodec, MetaCodec
from fqsqueezer_amd.fqsfile import compress_records, compress_records_pe
from fqsqueezer_amd.fqsread import decompress_fastq, decompress_fastq_chunks
from test_fqs_fastq import REF_FILES

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
TEXT = [pytest.param(True, id="gpu_text"), pytest.param(False, id="host_text")]


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


def _fixture(tag):
    d = json.load(open(os.path.join(GOLD, tag + ".json")))
    return d, open(os.path.join(GOLD, d["fqs"]), "rb").read()


def _streamed(src, paired, **kw):
    """the chunks joined per mate, and how many there were"""
    parts, n = ([], []), 0
    for chunk in decompress_fastq_chunks(src, device=0, **kw):
        assert isinstance(chunk, tuple) == paired and (not paired or len(chunk) == 2)
        for m, part in enumerate(chunk if paired else (chunk,)):
            assert isinstance(part, bytes)
            parts[m].append(part)
        n += 1
    return (b"".join(parts[0]), b"".join(parts[1])) if paired else b"".join(parts[0]), n


def _check_digests(d, text):
    for m, t in enumerate(text if d["paired"] else (text,)):
        ref = d["mate%d" % (m + 1)]
        assert len(t) == ref["fastq_bytes"] and hashlib.sha256(t).hexdigest() == ref["fastq_sha256"], f"mate {m + 1}: FASTQ text differs from `fqs d`"


# ---- 1. the reference's files ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("gpu_text", TEXT)
@pytest.mark.parametrize("tag", REF_FILES)
def test_reference_file_streams_to_the_text_fqs_d_writes(where, request, tag, gpu_text):
    d, data = _fixture(tag)
    st = {}
    text, n = _streamed(data, d["paired"], lib_path=_lib(where, request), gpu_text=gpu_text, stats=st)
    _check_digests(d, text)
    assert n == len(hp.parse_fqs(data)[1]) == st["text"]["blocks"]
    assert st["text"]["gpu_text"] is gpu_text
    assert st["text"]["bytes"] == [len(t) for t in (text if d["paired"] else (text, b""))]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("gpu_text", TEXT)
@pytest.mark.parametrize("tag", ["c24_c10_full_o_t3", "c24_c11_pe_s_i_t2"])
def test_the_host_id_decoder_feeds_either_assembly(where, request, tag, gpu_text):
    """gpu_ids=False: the ids come from the host decoder from the first block on, as host arrays"""
    d, data = _fixture(tag)
    st = {}
    text, n = _streamed(data, d["paired"], lib_path=_lib(where, request), gpu_ids=False, gpu_text=gpu_text, stats=st)
    _check_digests(d, text)
    assert n == len(hp.parse_fqs(data)[1]) and st["id_host_fallback"] is False and "id_decoder" not in st


# ---- 2. the files this library writes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order,qmode,imode", [("o", "lossless", "lossless"), ("s", "lossless", "lossless"), ("o", "illumina_8", "instrument"),
                                               ("s", "illumina_8", "instrument"), ("s", "none", "none")])
def test_own_files_stream_to_what_decompress_fastq_gives(where, request, order, qmode, imode):
    lib = _lib(where, request)
    files = [(compress_records(c4_records(), 4, order, 1, lib_path=lib, quality_mode=qmode, id_mode=imode), False)]
    r1, r2 = (hp.Records(r.ids[:1500], r.seq[:1500], r.qual[:1500]) for r in c5_records())
    files.append((compress_records_pe(r1, r2, 3, order, 1, lib_path=lib, quality_mode=qmode, id_mode=imode), True))
    for data, paired in files:
        want = decompress_fastq(data, device=0, lib_path=lib)
        got, n = _streamed(data, paired, lib_path=lib)
        assert got == want and n == len(hp.parse_fqs(data)[1])


# ---- 3. ids beyond the id kernel's staging limits ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_long_ids_stream_through_the_host_decoder(where, request):
    lib = _lib(where, request)
    rec = c4_records()
    ids = list(rec.ids)
    target = int(hp.form_blocks(rec, "se_sorted", exact_ties=True)[-1][0])   # a read of the last bin
    ids[target] = b"@long." + b"x" * 1500 + b".7"
    rec = hp.Records(ids, rec.seq, rec.qual)
    data = compress_records(rec, 3, "s", 1, lib_path=lib, quality_mode="none", id_mode="lossless")
    blks = hp.form_blocks(rec, "se_sorted", exact_ties=True)
    assert len(blks) > 1 and target not in blks[0]   # the blocks before it come from the device, the rest as host arrays
    st = {}
    got, n = _streamed(data, False, lib_path=lib, stats=st)
    assert n == len(blks) and st["id_host_fallback"] is True
    assert got == decompress_fastq(data, device=0, lib_path=lib) and ids[target] + b"\n" in got


# ---- 4. the id decoder runs blocks again ------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag", ["c24_c10_full_o_t3", "c24_c11_pe_s_i_t2"])
def test_device_resident_ids_survive_the_run_again_path(where, request, monkeypatch, tag):
    monkeypatch.setenv("FQSX_IDG_INIT", "1")
    d, data = _fixture(tag)
    st = {}
    text, _ = _streamed(data, d["paired"], lib_path=_lib(where, request), stats=st)
    _check_digests(d, text)
    assert st["id_host_fallback"] is False and st["id_decoder"]["retries"] >= 1, st


# ---- 5. the decoders' device entry points, block for block ------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("tag,min_blocks", [("c24_c10_full_o_t3", 1), ("c24_c10_s_i_t4", 2)])   # (the sorted file: the state moves on from block to block)
def test_decode_block_dev_equals_decode_block(where, request, tag, min_blocks):
    lib = _lib(where, request)
    _, data = _fixture(tag)
    header, blocks = hp.parse_fqs(data)
    T, paired = header[4], header[5] >= 2
    meta = MetaCodec(T, lib_path=lib)
    dna_h, dna_d = (DnaCodec(header, device=0, lib_path=lib) for _ in range(2))
    id_h, id_d = (IdCodec(header, lib_path=lib, device=0) for _ in range(2))
    mem = DeviceColumns(device=0, lib_path=lib)   # (an empty store: its download reads any device memory back)
    try:
        assert len(blocks) >= min_blocks
        for g, blk in enumerate(blocks):
            st = lambda sid: [blk.streams[w][sid] for w in range(T)]   # noqa: E731
            read_len = meta.decode_block(st(hp.STREAM_META), blk.n_reads, paired)
            off = np.concatenate([[0], np.cumsum(read_len, dtype=np.uint64)]).astype(np.uint64)
            bases = dna_h.decode_block(st(hp.STREAM_DNA), off, g)
            ids, id_off = id_h.decode_block(st(hp.STREAM_ID), blk.n_reads, paired)
            d_bases = dna_d.decode_block_dev(st(hp.STREAM_DNA), off, g)
            d_ids, d_len, id_bytes = id_d.decode_block_dev(st(hp.STREAM_ID), blk.n_reads, paired)
            assert d_bases and d_ids and d_len
            assert mem.download(d_bases, int(off[-1])).tobytes() == bases.tobytes(), f"block {g}: bases"
            assert id_bytes == len(ids) and mem.download(d_ids, id_bytes).tobytes() == ids.tobytes(), f"block {g}: id lines"
            assert np.array_equal(mem.download(d_len, 4 * blk.n_reads).view(np.uint32), np.diff(id_off.astype(np.int64))), f"block {g}: id lengths"
    finally:
        for c in (meta, dna_h, dna_d, id_h, id_d, mem):
            c.close()


# ---- 6. bounded reading -----------------------------------------------------------------------------------------------------
class CountingFile:
    def __init__(self, data):
        self.f, self.handed_out, self.largest = io.BytesIO(data), 0, 0

    def read(self, n=-1):
        b = self.f.read(n)
        self.handed_out += len(b)
        self.largest = max(self.largest, len(b))
        return b


def test_iter_fqs_reads_no_further_than_a_piece_past_the_block():
    _, data = _fixture("c24_c10_s_i_t4")
    header, blocks = hp.parse_fqs(data)
    ends, pos = [], 18
    for chunk in list(hp.fqs_chunks(header, blocks))[1:]:
        pos += len(chunk)
        ends.append(pos)
    assert pos == len(data) and len(blocks) >= 3
    f = CountingFile(data)
    it = hp.iter_fqs(f, read_size=4096)
    assert next(it) == header and f.handed_out <= 18 + 4096
    got = []
    for k, blk in enumerate(it):
        assert f.handed_out <= ends[k] + 4096, f"block {k}"
        got.append(blk)
    assert got == blocks and f.largest <= 4096 and f.handed_out == len(data)


@pytest.mark.parametrize("cut", ["in_a_stream", "in_a_varint", "after_the_first_block_header"])
def test_iter_fqs_refuses_a_file_cut_inside_a_block(cut):
    _, data = _fixture("c24_c10_s_i_t4")
    header, blocks = hp.parse_fqs(data)
    first_end = 18 + len(list(hp.fqs_chunks(header, blocks))[1])
    at = {"in_a_stream": first_end + (len(data) - first_end) // 2, "in_a_varint": first_end + 1, "after_the_first_block_header": 18 + 2}[cut]
    it = hp.iter_fqs(io.BytesIO(data[:at]), read_size=4096)
    assert next(it) == header
    with pytest.raises(ValueError, match="ends inside a block"):
        list(it)
    for bad in (b"", b"\x10" + data[1:], data[:1] + b"XXXX" + data[5:], data[:10]):
        with pytest.raises(ValueError, match="not a .fqs file"):
            next(hp.iter_fqs(io.BytesIO(bad)))


# ---- 7. the command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-host-text"]], ids=["gpu_text", "host_text"])
def test_command_line_streams_the_file(built, tmp_path, flags):
    from fqsqueezer_amd import fqsread
    d = json.load(open(os.path.join(GOLD, "c24_c11_pe_o_o_t3.json")))
    o1, o2 = tmp_path / "a.fq", tmp_path / "b.fq"
    assert fqsread.main(["d", os.path.join(GOLD, d["fqs"]), "-out", str(o1), "-out2", str(o2), "-lib", EMU_LIB] + flags) == 0
    assert hashlib.sha256(o1.read_bytes()).hexdigest() == d["mate1"]["fastq_sha256"]
    assert hashlib.sha256(o2.read_bytes()).hexdigest() == d["mate2"]["fastq_sha256"]


def test_command_line_refuses_a_paired_file_without_out2(built, tmp_path):
    from fqsqueezer_amd import fqsread
    d = json.load(open(os.path.join(GOLD, "c24_c11_pe_o_o_t3.json")))
    o1 = tmp_path / "a.fq"
    with pytest.raises(SystemExit) as e:
        fqsread.main(["d", os.path.join(GOLD, d["fqs"]), "-out", str(o1), "-lib", EMU_LIB])
    assert e.value.code != 0
    assert not o1.exists() or o1.stat().st_size == 0
