"""gzip-compressed FASTQ through codec.parse_fastq, compress_fastq and `e`: BGZF inflated on the device (members straight into
the parser's buffer, the partial record carried there), any gzip through zlib on the host -- always the columns, and the .fqs
bytes, of the plain text.  Emulation build and, marked gpu, device 0."""
import functools
import gzip

import numpy as np
import pytest

from test_bgzf_inflate import EOF_MEMBER, bgzf, deflate, member
from test_fastq_parse import texts as parse_texts
from test_fqs_compress import WHERE, _lib, texts
from fqsqueezer_amd import fqsfile
from fqsqueezer_amd.codec import parse_fastq
from fqsqueezer_amd.fqsfile import compress_fastq

CHUNK = 2 * 65280 + 100   # two members of 65280 bytes fit unless the carried record is longer than 100 bytes: chunks of one member and of two
NAMES = ["c4", "c7", "empty_fields"]
COLS = ["ids", "id_off", "bases", "read_off", "quals", "qual_off"]


def same_columns(a, b):
    assert len(a) == len(b)
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.plus_len is None and b.plus_len is None) or np.array_equal(a.plus_len, b.plus_len)


@functools.lru_cache(maxsize=None)
def plain(name: str, lib):
    st = {}
    return parse_fastq(parse_texts(name), lib_path=lib, stats=st), st


def check(src, name: str, lib, fmt: str, where: str, **kw):
    st = {}
    want, want_st = plain(name, lib)
    same_columns(parse_fastq(src, lib_path=lib, stats=st, **kw), want)
    for k in ("consumed", "tail_bytes", "max_id_line", "length_mismatch"):
        assert st[k] == want_st[k], k
    assert st["inflate"]["format"] == fmt and st["inflate"]["where"] == where and st["inflate"]["members"] > 0
    assert want_st["inflate"] == {"format": "none", "where": "host", "members": 0, "compressed_bytes": 0}
    return st


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", NAMES)
def test_bgzf_bytes_and_path_parse_to_the_columns_of_the_text(where, request, name, tmp_path):
    lib, text = _lib(where, request), parse_texts(name)
    gz = bgzf(text)
    st = check(gz, name, lib, "bgzf", "device", max_chunk_bytes=CHUNK, inflate="device")
    n_members = -(-len(text) // 65280) + 1
    assert st["inflate"]["members"] == n_members and st["inflate"]["compressed_bytes"] == len(gz)
    if len(text) > 4 * 65280:   # records straddle members and chunks; chunks of one member and chunks of two
        assert len(text) % 65280 and n_members / 2 < st["chunks"] < n_members
    f = tmp_path / "reads.fastq"   # (told by its bytes, not by its name)
    f.write_bytes(gz)
    check(str(f), name, lib, "bgzf", "device", max_chunk_bytes=CHUNK, inflate="device", profile=True)
    check(np.frombuffer(gz, dtype=np.uint8), name, lib, "bgzf", "device")   # one chunk
    # small members, several records in none of them whole
    check(bgzf(text, member_bytes=777, level=1), name, lib, "bgzf", "device", max_chunk_bytes=1 << 12)


@pytest.mark.parametrize("where", WHERE)
def test_the_tail_behind_the_last_record_is_reported_as_for_text(where, request):
    lib = _lib(where, request)
    text = parse_texts("c4")[:200000] + b"@partial\nACGT\n+"
    want, got = {}, {}
    a = parse_fastq(text, lib_path=lib, stats=want)
    b = parse_fastq(bgzf(text), lib_path=lib, stats=got, max_chunk_bytes=CHUNK, inflate="device")
    same_columns(a, b)
    assert got["tail_bytes"] == want["tail_bytes"] > 0 and got["consumed"] == want["consumed"]
    for inflate in ("device", "host"):
        st = {}
        assert len(parse_fastq(bgzf(b"no record at all"), lib_path=lib, stats=st, inflate=inflate)) == 0 and st["tail_bytes"] == 16
        assert len(parse_fastq(EOF_MEMBER, lib_path=lib, stats=st, inflate=inflate)) == 0 and st["tail_bytes"] == 0


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", NAMES)
def test_the_host_path_and_plain_gzip_parse_to_the_columns_of_the_text(where, request, name, tmp_path):
    lib, text = _lib(where, request), parse_texts(name)
    check(bgzf(text), name, lib, "bgzf", "host", max_chunk_bytes=CHUNK, inflate="host")
    st = check(gzip.compress(text), name, lib, "gzip", "host", max_chunk_bytes=CHUNK)
    assert st["inflate"]["members"] == 1
    cut = text.index(b"\n", len(text) // 2) - 3   # two gzip files concatenated, cut inside a line
    two = gzip.compress(text[:cut], 1) + gzip.compress(text[cut:], 9)
    f = tmp_path / "two.gz"
    f.write_bytes(two)
    st = check(str(f), name, lib, "gzip", "host", max_chunk_bytes=CHUNK, inflate="auto")
    assert st["inflate"]["members"] == 2 and st["inflate"]["compressed_bytes"] == len(two)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("ids", [False, True], ids=["resident", "resident_ids"])
def test_resident_columns_from_bgzf(where, request, ids):
    lib, text = _lib(where, request), parse_texts("c4")
    st = {}
    a = parse_fastq(text, lib_path=lib, max_chunk_bytes=CHUNK, resident=True, resident_ids=ids)
    b = parse_fastq(bgzf(text), lib_path=lib, max_chunk_bytes=CHUNK, resident=True, resident_ids=ids, stats=st, inflate="device")
    try:
        assert st["inflate"]["format"] == "bgzf" and st["inflate"]["where"] == "device"
        assert len(a) == len(b) and a.info()["bases"] == b.info()["bases"]
        assert np.array_equal(a.bases_to_host(), b.bases_to_host()) and np.array_equal(a.read_off, b.read_off)
        idx = np.arange(len(a) - 1, -1, -7)
        blk_a, blk_b = a.block_dev(idx), b.block_dev(idx)
        assert np.array_equal(blk_a.off, blk_b.off)
        n = int(blk_a.off[-1])
        assert np.array_equal(a.download(blk_a.quals, n), b.download(blk_b.quals, n))
        for x, y in zip(a.ids_of(idx), b.ids_of(idx)):
            assert np.array_equal(x, y)
        if ids:
            assert a.id_survey() == b.id_survey() and b.id_survey()["id_bytes"] > 0 and len(b.ids) == 0
    finally:
        a.close()
        b.close()


@functools.lru_cache(maxsize=None)
def small(paired: bool):
    if not paired:
        t = texts("c4")
        return (t[:t.index(b"\n@rag.801\n") + 1],)
    t1, t2 = (t[:t.index(b"\n", 150000) + 1] for t in texts("c5"))
    return tuple(t[:t.rindex(b"\n@", 0, len(t) - 1) + 1] for t in (t1, t2))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("order", ["o", "s"])
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_compress_fastq_on_gz_input_gives_the_bytes_of_the_text(where, request, paired, order):
    kw = dict(threads=2, order=order, genome_size_mbp=1, lib_path=_lib(where, request))
    t = small(paired)
    want = compress_fastq(*t, **kw)
    st = {}
    assert compress_fastq(*(bgzf(x, member_bytes=30011) for x in t), max_chunk_bytes=CHUNK, stats=st, inflate="device", **kw) == want
    assert [s["inflate"]["where"] for s in st["parse"]] == ["device"] * len(t)
    assert compress_fastq(*(gzip.compress(x) for x in t), inflate="auto", **kw) == want
    if paired:   # each mate on its own
        assert compress_fastq(bgzf(t[0]), t[1], stats=st, inflate="device", **kw) == want
        assert [s["inflate"]["format"] for s in st["parse"]] == ["bgzf", "none"]
        assert compress_fastq(t[0], gzip.compress(t[1]), resident=True, **kw) == want


@pytest.mark.parametrize("where", WHERE)
def test_command_line_e_on_a_bgzf_path(where, request, tmp_path):
    lib = _lib(where, request)
    extra = ["-lib", lib] if lib else []
    (se,) = small(False)
    src, out = tmp_path / "se.fq.gz", tmp_path / "se.fqs"
    src.write_bytes(bgzf(se))
    want = compress_fastq(se, threads=2, order="o", genome_size_mbp=1, quality_mode="lossless", id_mode="lossless", lib_path=lib)
    for flags in (["-inflate", "device"], ["-inflate", "host"], ["-resident-ids"]):
        assert fqsfile.main(["e", "-s", "-om", "o", "-t", "2", "-gs", "1", "-qm", "o", "-im", "o", "-out", str(out), str(src)] + flags + extra) == 0
        assert out.read_bytes() == want


@pytest.mark.parametrize("where", WHERE)
def test_errors(where, request, tmp_path):
    lib, text = _lib(where, request), parse_texts("c7")[:150000]
    gz = bgzf(text, member_bytes=20000)
    parts = [member(deflate(text[i:i + 20000]), text[i:i + 20000]) for i in range(0, len(text), 20000)]
    assert b"".join(parts) + EOF_MEMBER == gz
    for inflate in ("device", "host"):
        for cut in (len(parts[0]) + 9, len(parts[0]) + len(parts[1]) // 2, len(gz) - 30):   # inside a header, inside deflate data, inside a trailer
            with pytest.raises(ValueError, match="cut short"):
                parse_fastq(gz[:cut], lib_path=lib, inflate=inflate)
        with pytest.raises(ValueError):
            parse_fastq(gz + b"garbage behind the last member", lib_path=lib, inflate=inflate)
    bad = bytearray(gz)
    at = sum(len(p) for p in parts[:3])
    bad[at + 18 + len(parts[3]) // 2] ^= 0x10
    for src in (bytes(bad), None):
        if src is None:
            src = str(tmp_path / "bad.gz")
            open(src, "wb").write(bad)
        with pytest.raises(ValueError, match=r"member 3 at offset %d is damaged: \w" % at):
            parse_fastq(src, lib_path=lib, inflate="device", max_chunk_bytes=1 << 15)
    with pytest.raises(ValueError, match="device"):
        parse_fastq(gzip.compress(text), lib_path=lib, inflate="device")
    with pytest.raises(ValueError):
        parse_fastq(gz, lib_path=lib, inflate="gpu")
    # without bgzip's end-of-file member: nothing wrong
    same = parse_fastq(text, lib_path=lib)
    for inflate in ("device", "host"):
        st = {}
        same_columns(parse_fastq(bgzf(text, member_bytes=20000, eof=False), lib_path=lib, inflate=inflate, stats=st), same)
        assert st["inflate"]["members"] == len(parts)
