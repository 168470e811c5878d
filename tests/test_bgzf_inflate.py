"""The BGZF inflate kernel (fqsx_bgzf_inflate) against zlib, byte for byte, and the member scan (fqsx_bgzf_scan).

The module builds its BGZF members itself: a header written by hand around zlib.compressobj(level, DEFLATED, -15, memLevel,
strategy), or around deflate data assembled bit by bit here.  py_inflate() below is the specification of raw DEFLATE (RFC 1951):
it is checked against zlib.decompress, and it reports what a stream contains -- block types, longest code, largest distance,
longest match, whether a match overlaps its own output -- so that every group can assert that its inputs hold what it is
about.  Damaged members are judged by zlib on the host plus the CRC-32 and ISIZE of the trailer.  Emulation build and, marked
gpu, device 0."""
import functools
import gzip
import struct
import zlib

import numpy as np
import pytest

from conftest import EMU_LIB, c4_records
from fqsqueezer_amd.codec import FastqParser, FqsxError, bgzf_inflate, bgzf_scan
from fqsqueezer_amd.synth import fastq_text

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # bgzip's 28-byte end-of-file member


def _lib(where, request):
    if where == "emu":
        request.getfixturevalue("built")
        return EMU_LIB
    return None


# ---------------------------------------------------------------------------------------------------------- building members
def member(deflate: bytes, text: bytes = None, crc: int = None, isize: int = None, extra_before: bytes = b"") -> bytes:
    """a BGZF member around raw deflate data; the trailer is that of `text` unless given.  (65536 bytes of text that do not
    compress make a member longer than BSIZE can say: fqsx_bgzf_inflate, which is told where a member ends, takes it all the
    same; a file cannot hold it, and bgzf() below refuses to build one.)"""
    xlen = len(extra_before) + 6
    size = 12 + xlen + len(deflate) + 8
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\x00" + struct.pack("<H", (size - 1) & 0xffff)
    crc = zlib.crc32(text) if crc is None else crc
    isize = len(text) if isize is None else isize
    return head + deflate + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def deflate(text: bytes, level: int = 6, mem_level: int = 8, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(text) + c.flush()


def bgzf(text: bytes, member_bytes: int = 65280, eof: bool = True, **enc) -> bytes:
    """a BGZF file of text: members of member_bytes of text each, and bgzip's empty member at the end"""
    parts = [member(deflate(text[i:i + member_bytes], **enc), text[i:i + member_bytes]) for i in range(0, len(text), member_bytes)]
    assert all(len(m) <= 65536 for m in parts)
    return b"".join(parts) + (EOF_MEMBER if eof else b"")


class Bits:
    """deflate data assembled by hand: fixed-Huffman blocks of literals and matches"""
    LEN = [(3 + k, 0) for k in range(8)] + [(((k - 4) % 4 + 4 << (k - 4) // 4) + 3, (k - 4) // 4) for k in range(8, 28)] + [(258, 0)]
    DIST = [(1 + k, 0) for k in range(4)] + [((k % 2 + 2 << k // 2 - 1) + 1, k // 2 - 1) for k in range(4, 30)]

    def __init__(self):
        self.acc = self.n = 0
        self.out = bytearray()

    def put(self, value: int, n: int):   # n bits, least significant first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int):   # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % n)[::-1], 2), n)

    def block(self, last: bool, btype: int = 1):
        self.put(int(last), 1)
        self.put(btype, 2)

    def symbol(self, s: int):   # literal/length symbol of the fixed code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xc0 + s - 280, 8)

    def match(self, length: int, dist: int):
        k = max(i for i, (b, _) in enumerate(self.LEN) if b <= length and (i < 28 or length == 258))
        self.symbol(257 + k)
        self.put(length - self.LEN[k][0], self.LEN[k][1])
        k = max(i for i, (b, _) in enumerate(self.DIST) if b <= dist)
        self.code(k, 5)
        self.put(dist - self.DIST[k][0], self.DIST[k][1])

    def done(self) -> bytes:
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


# ------------------------------------------------------------------------------------------------------- the specification
class Report(dict):
    pass


def py_inflate(data: bytes, limit: int = 1 << 17):
    """(text, report) of raw deflate data; ValueError for anything RFC 1951 does not allow.  Plain and slow on purpose."""
    pos = [0]

    def bits(n: int) -> int:
        v = 0
        for k in range(n):
            if pos[0] >= 8 * len(data):
                raise ValueError("input exhausted")
            v |= (data[pos[0] >> 3] >> (pos[0] & 7) & 1) << k
            pos[0] += 1
        return v

    def table(lens):
        """{(length, code): symbol} of the canonical code"""
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        left = 1
        for l in range(1, 16):
            left = 2 * left - count[l]
            if left < 0:
                raise ValueError("over-subscribed code")
        code, nxt = 0, [0] * 16
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        t = {}
        for s, l in enumerate(lens):
            if l:
                t[(l, nxt[l])] = s
                nxt[l] += 1
        return t, left

    def decode(t) -> int:
        code = 0
        for l in range(1, 16):
            code = code << 1 | bits(1)
            if (l, code) in t:
                return t[(l, code)]
        raise ValueError("invalid symbol")

    out = bytearray()
    rep = Report(types=[], max_code=0, max_dist=0, max_len=0, overlap=False, matches=0)
    fixed = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)[0], table([5] * 30)[0]
    last = 0
    while not last:
        last, btype = bits(1), bits(2)
        rep["types"].append(btype)
        if btype == 3:
            raise ValueError("reserved block type")
        if btype == 0:
            pos[0] = (pos[0] + 7) & ~7
            n, nn = bits(16), bits(16)
            if n ^ 0xffff != nn:
                raise ValueError("stored LEN/NLEN mismatch")
            if (pos[0] >> 3) + n > len(data):
                raise ValueError("input exhausted")
            out += data[pos[0] >> 3:(pos[0] >> 3) + n]
            pos[0] += 8 * n
            continue
        if btype == 1:
            lt, dt = fixed
        else:
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            if hlit > 286 or hdist > 30:
                raise ValueError("too many codes")
            cl = [0] * 19
            for k in range(hclen):
                cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][k]] = bits(3)
            ct, left = table(cl)
            if left:
                raise ValueError("incomplete code")
            lens = []
            while len(lens) < hlit + hdist:
                s = decode(ct)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16 and not lens:
                    raise ValueError("repeat without a length")
                r, v = (3 + bits(2), lens[-1]) if s == 16 else (3 + bits(3), 0) if s == 17 else (11 + bits(7), 0)
                lens += [v] * r
            if len(lens) > hlit + hdist:
                raise ValueError("repeat beyond the lengths")
            if not lens[256]:
                raise ValueError("no end-of-block code")
            (lt, l_left), (dt, d_left) = table(lens[:hlit]), table(lens[hlit:])
            if (l_left and max(lens[:hlit]) != 1) or (d_left and max(lens[hlit:]) > 1):
                raise ValueError("incomplete code")
            rep["max_code"] = max(rep["max_code"], max(lens))
        while True:
            s = decode(lt)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise ValueError("invalid symbol")
                base, extra = Bits.LEN[s - 257]
                n = base + bits(extra)
                ds = decode(dt)
                if ds > 29:
                    raise ValueError("invalid symbol")
                base, extra = Bits.DIST[ds]
                d = base + bits(extra)
                if d > len(out):
                    raise ValueError("distance before the start")
                for _ in range(n):
                    out.append(out[-d])
                rep.update(max_dist=max(rep["max_dist"], d), max_len=max(rep["max_len"], n), overlap=rep["overlap"] or d < n, matches=rep["matches"] + 1)
            if len(out) > limit:
                raise ValueError("output beyond the limit")
    return bytes(out), rep


def verdict(m: bytes):
    """the text of a member as zlib on the host gives it and its trailer confirms it, or None"""
    xlen = struct.unpack_from("<H", m, 10)[0]
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(m[12 + xlen:len(m) - 8])
    except zlib.error:
        return None
    crc, isize = struct.unpack("<II", m[-8:])
    return text if d.eof and zlib.crc32(text) == crc and len(text) == isize else None


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def fq_text() -> bytes:
    r = c4_records()
    return fastq_text(r.ids, [r.seq_bytes(i) for i in range(len(r))], [r.qual_bytes(i) for i in range(len(r))])


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def content(name: str) -> bytes:
    if name == "fastq":
        return fq_text()[:65536]
    if name == "one_byte":
        return b"G" * 65536
    if name.startswith("period"):
        p = int(name[6:])
        return (_rand(p, p) * (65536 // p + 1))[:40000]
    if name == "twice32768":
        return _rand(32768, 5) * 2
    if name == "random":
        return _rand(50001, 6)
    if name == "fibonacci":   # 245 byte values once each (a subtree 8 deep), 11 with Fibonacci frequencies from there: an unlimited Huffman code of 19 bits
        f = [245, 245]
        while len(f) < 11:
            f.append(f[-1] + f[-2])
        t = np.concatenate([np.full(n, 34 + k, dtype=np.uint8) for k, n in enumerate(f)] + [np.setdiff1d(np.arange(256), np.arange(34, 45)).astype(np.uint8)])
        return np.random.default_rng(7).permutation(t).tobytes()
    raise KeyError(name)


ENCODERS = {"stored": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED), "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9),
            "huffman": dict(strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(strategy=zlib.Z_RLE), "l9m1": dict(level=9, mem_level=1)}
SIZES = [0, 1, 65280, 65536]


@functools.lru_cache(maxsize=None)
def encoded(name: str, enc: str, size: int = None):
    """(deflate data, text, report) -- the report from py_inflate, which has to agree with zlib on the text"""
    text = content(name) if size is None else content(name)[:size]
    data = deflate(text, **ENCODERS[enc])
    out, rep = py_inflate(data)
    assert out == text == zlib.decompress(data, -15)
    return data, text, rep


def run(lib, members, expect=None):
    """the members through fqsx_bgzf_inflate in one call; their texts must be `expect` (default: what zlib says)"""
    blob = np.frombuffer(b"".join(members), dtype=np.uint8)
    off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64) if members else np.zeros(0, dtype=np.uint64)
    expect = [verdict(m) for m in members] if expect is None else expect
    p = FastqParser(0, lib)
    try:
        text = bgzf_inflate(p, blob, off, sum(struct.unpack("<I", m[-4:])[0] for m in members))
    finally:
        p.close()
    assert text.tobytes() == b"".join(expect)


def refused(lib, members, at: int):
    """the call must name member `at` as damaged; returns the kind"""
    blob = np.frombuffer(b"".join(members), dtype=np.uint8)
    off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64)
    p = FastqParser(0, lib)
    try:
        with pytest.raises(FqsxError) as e:
            bgzf_inflate(p, blob, off, sum(min(struct.unpack("<I", m[-4:])[0], 1 << 17) for m in members))
    finally:
        p.close()
    assert e.value.member == at and ("member %d " % at) in str(e.value) and e.value.kind in str(e.value)
    return e.value.kind


# ------------------------------------------------------------------------------------------------------------------- tests
def test_the_specification_agrees_with_zlib_and_sees_what_it_reports():
    b = Bits()
    b.block(True)
    for ch in b"abc":
        b.symbol(ch)
    b.match(258, 3)
    b.match(5, 2)
    b.symbol(256)
    text, rep = py_inflate(b.done())
    assert text == zlib.decompress(b.done(), -15) == b"abc" * 87 + b"bcbcb"
    assert rep == dict(types=[1], max_code=0, max_dist=3, max_len=258, overlap=True, matches=2)
    for bad in (b"\x07", b"\x01\x01\x00\x00\x00", b"\x03"):   # block type 3, NLEN mismatch, a fixed block cut before its end-of-block code
        with pytest.raises(ValueError):
            py_inflate(bad)
    assert member(deflate(b""), b"") == EOF_MEMBER and verdict(EOF_MEMBER) == b""


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("enc", list(ENCODERS))
def test_sizes_under_every_encoder(where, request, enc):
    cases = [encoded("fastq", enc, n) for n in SIZES]
    types = [set(rep["types"]) for _, _, rep in cases]
    if enc == "stored":   # (a stored block holds 65535 bytes at most)
        assert all(t == {0} for t in types) and len(cases[3][2]["types"]) >= 2
    elif enc == "fixed":
        assert all(t == {1} for t in types)
    else:
        assert 2 in types[2] and 2 in types[3]
    if enc == "l9m1":   # the tables are rebuilt many times in one member
        assert len(cases[3][2]["types"]) >= 8
    if enc == "huffman":
        assert cases[3][2]["matches"] == 0
    if enc == "rle":
        assert cases[3][2]["max_dist"] <= 1
    run(_lib(where, request), [member(d, t) for d, t, _ in cases], [t for _, t, _ in cases])


@pytest.mark.parametrize("where", WHERE)
def test_the_empty_member_alone(where, request):
    run(_lib(where, request), [EOF_MEMBER], [b""])
    run(_lib(where, request), [], [])


CONTENTS = [("one_byte", "l6"), ("one_byte", "fixed"), ("period3", "l9"), ("period63", "l9"), ("period64", "l9"), ("period65", "l9"), ("period127", "l9"),
            ("period64", "fixed"), ("twice32768", "l9"), ("twice32768", "hand"), ("random", "l6"), ("random", "huffman"), ("fibonacci", "huffman"),
            ("fibonacci", "l6")]


@functools.lru_cache(maxsize=None)
def twice32768_by_hand():
    """32768 literals, then matches at distance 32768 (zlib itself never looks back further than 32506)"""
    text = content("twice32768")
    b = Bits()
    b.block(True)
    for ch in text[:32768]:
        b.symbol(ch)
    left = 32768
    while left:
        n = 258 if left >= 261 or left == 258 else left if left < 258 else left - 3
        b.match(n, 32768)
        left -= n
    b.symbol(256)
    data = b.done()
    out, rep = py_inflate(data)
    assert out == text == zlib.decompress(data, -15)
    return data, text, rep


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,enc", CONTENTS)
def test_contents(where, request, name, enc):
    data, text, rep = twice32768_by_hand() if enc == "hand" else encoded(name, enc)
    if name == "one_byte":
        assert rep["max_len"] == 258 and rep["max_dist"] == 1 and rep["overlap"]
    if name.startswith("period"):
        assert rep["max_dist"] == int(name[6:]) and rep["max_len"] == 258 and rep["overlap"]   # out[p + k] = out[p - d + k mod d], d on either side of 64
    if enc == "hand":
        assert rep["max_dist"] == 32768 and rep["max_len"] == 258
    if name == "twice32768" and enc == "l9":
        assert rep["max_dist"] <= 32506   # (zlib never looks back further: the distance 32768 is assembled by hand)
    if name == "fibonacci":
        assert (rep["max_code"] == 15 or enc != "huffman") and rep["max_code"] > 10 and len(set(text)) == 256   # (beyond the lookup table's bits)
    if name == "random":
        assert len(text) % 64 and (rep["matches"] == 0 or enc == "l6")
    run(_lib(where, request), [member(data, text)], [text])


@functools.lru_cache(maxsize=None)
def many_members():
    rng = np.random.default_rng(11)
    sizes = [0, 65536, 1, 65280, 0, 65535] + [int(x) for x in rng.integers(0, 20000, 290)] + [65536, 0, 3, 65536]
    src = fq_text() + content("random") + content("period65")
    encs = list(ENCODERS.values())
    texts = [src[(7919 * i) % 100000:][:n] for i, n in enumerate(sizes)]
    assert [len(t) for t in texts] == sizes and len(sizes) == 300
    return [member(deflate(t, **encs[i % len(encs)]), t) for i, t in enumerate(texts)], texts


@pytest.mark.parametrize("where", WHERE)
def test_three_hundred_members_each_at_its_own_offset(where, request):
    members, texts = many_members()
    run(_lib(where, request), members, texts)


# ------------------------------------------------------------------------------------------------------------------ damage
@functools.lru_cache(maxsize=None)
def small(kind: str):
    """(deflate data, text) of the small member that gets damaged"""
    text = fq_text()[1000:1700]
    data = deflate(text, level=0 if kind == "stored" else 6)
    assert set(py_inflate(data)[1]["types"]) == ({0} if kind == "stored" else {2})
    return data, text


def neighbours():
    return member(*encoded("fastq", "l6", 65280)[:2]), member(*encoded("fastq", "fixed", 1)[:2])


def judge(lib, m: bytes):
    """member m between two good ones: refused by name where zlib refuses it, its text where zlib accepts it"""
    a, b = neighbours()
    v = verdict(m)
    if v is None:
        return refused(lib, [a, m, b], 1)
    run(lib, [a, m, b], [verdict(a), v, verdict(b)])
    return None


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", ["dynamic", "stored"])
def test_two_hundred_bit_flips(where, request, kind):
    data, text = small(kind)
    lib = _lib(where, request)
    rng = np.random.default_rng(3 if kind == "stored" else 4)
    first = 48 if kind == "stored" else 120   # the block header and LEN / NLEN, or the code lengths' beginning: every bit; then seeded ones
    flips = (list(range(first)) + sorted(set(int(x) for x in rng.integers(first, 8 * len(data), 230))))[:200]
    assert len(flips) == 200
    kinds, harmless = set(), 0
    for bit in flips:
        d = bytearray(data)
        d[bit >> 3] ^= 1 << (bit & 7)
        k = judge(lib, member(bytes(d), text))
        harmless += k is None
        kinds.add(k)
    assert harmless <= 8 and len(kinds - {None}) >= (3 if kind == "dynamic" else 2)   # (only a stream's padding bits do not matter)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", ["dynamic", "stored"])
def test_damage_by_hand(where, request, kind):
    data, text = small(kind)
    lib = _lib(where, request)
    crc = zlib.crc32(text)
    assert judge(lib, member(data, text)) is None
    for cut in (1, 2, len(data) // 2, len(data) - 1):
        k = judge(lib, member(data[:len(data) - cut], text))
        assert k == "input exhausted" or (k is not None and cut > 2)
    assert judge(lib, member(data, text, isize=len(text) + 1)) == "ISIZE mismatch"
    assert judge(lib, member(data, text, isize=len(text) - 1)) in ("ISIZE mismatch", "output beyond ISIZE")
    assert judge(lib, member(data, text, crc=crc ^ 0x00100000)) == "CRC mismatch"
    assert judge(lib, member(bytes([data[0] | 6]) + data[1:], text)) == "reserved block type"
    full = encoded("fastq", "l6" if kind == "dynamic" else "stored", 65536)
    assert judge(lib, member(full[0], full[1], isize=65537)) == "ISIZE mismatch"
    if kind == "stored":
        assert judge(lib, member(data[:3] + bytes([data[3] ^ 1]) + data[4:], text)) == "stored LEN/NLEN mismatch"
    else:
        b = Bits()
        b.block(True)
        b.match(3, 1)
        b.symbol(256)
        assert judge(lib, member(b.done(), b"AAA")) == "distance before the member's start"
        b = Bits()
        b.block(True)
        b.symbol(65)
        b.match(258, 1)
        b.symbol(256)
        assert judge(lib, member(b.done(), b"A" * 200)) == "output beyond ISIZE"
        b = Bits()
        b.block(True)
        b.symbol(286)
        assert judge(lib, member(b.done(), b"")) == "invalid symbol"


# -------------------------------------------------------------------------------------------------------------------- scan
@pytest.mark.parametrize("where", WHERE)
def test_scan(where, request):
    lib = _lib(where, request)
    d, t, _ = encoded("fastq", "l6", 1000)
    ms = [member(d, t, extra_before=b"XY\x03\x00abc"), member(d, t), EOF_MEMBER, member(d, t, extra_before=b"BX\x02\x00zz" + b"ZZ\x00\x00")]
    blob = b"".join(ms)
    scan = lambda b, **kw: bgzf_scan(np.frombuffer(b, dtype=np.uint8), lib, **kw)
    off, isize, span, tail, bad = scan(blob)
    assert list(off) == list(np.cumsum([0] + [len(m) for m in ms[:-1]])) and list(isize) == [1000, 1000, 0, 1000]
    assert (span, tail, bad) == (len(blob), 0, False)
    run(lib, ms, [t, t, b"", t])
    for cut in (len(ms[0]) + 5, len(ms[0]) + 11, len(ms[0]) + 17, len(ms[0]) + 40, len(ms[0]) + len(ms[1]) - 1):   # inside a header, inside the deflate data, inside the trailer
        off, isize, span, tail, bad = scan(blob[:cut])
        assert (len(off), span, tail, bad) == (1, len(ms[0]), cut - len(ms[0]), False)
    assert scan(blob, max_members=2)[2:] == (len(ms[0]) + len(ms[1]), len(ms[2]) + len(ms[3]), False)
    off, isize, span, tail, bad = scan(ms[1] + gzip.compress(t))
    assert (len(off), span, bad) == (1, len(ms[1]), True)
    assert scan(gzip.compress(t))[2:] == (0, len(gzip.compress(t)), True)
    assert scan(b"@r1\nACGT\n+\nIIII\n")[4] and scan(b"\x1f")[2:] == (0, 1, False) and scan(b"")[2:] == (0, 0, False)
    no_bc = bytearray(ms[1])
    no_bc[12:14] = b"XX"
    assert scan(bytes(no_bc))[2:] == (0, len(no_bc), True)
