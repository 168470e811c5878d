"""Seeded synthetic FASTQ generator (SURVEY.md §8d workload definition).

Uniform-random genome of length G, reads sampled uniformly, strand 50/50,
per-base substitution 0.5 %, N 0.1 %, ids ``@SRR000001.<i> <i>/1``, qualities
iid from {2,14,22,27,33,37,40}+33.  Deterministic for a given
(n_reads, read_len, genome_len, seed) and numpy version-independent
(uses only PCG64 integer/uniform draws).
"""
from __future__ import annotations

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b
_QUALS = np.array([2, 14, 22, 27, 33, 37, 40], dtype=np.uint8) + 33


def synth_reads(n_reads: int, read_len: int, genome_len: int, seed: int,
                sub_rate: float = 0.005, n_rate: float = 0.001) -> np.ndarray:
    """Return an (n_reads, read_len) uint8 array of ASCII bases (ACGTN)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = _ACGT[rng.integers(0, 4, size=genome_len, dtype=np.uint8)]
    out = np.empty((n_reads, read_len), dtype=np.uint8)
    chunk = 1 << 18
    ar = np.arange(read_len, dtype=np.int64)
    for s in range(0, n_reads, chunk):
        e = min(n_reads, s + chunk)
        m = e - s
        pos = rng.integers(0, genome_len - read_len + 1, size=m, dtype=np.int64)
        strand = rng.integers(0, 2, size=m, dtype=np.uint8)
        r = genome[pos[:, None] + ar[None, :]]
        rc = _COMP[r[:, ::-1]]
        r = np.where(strand[:, None] == 1, rc, r)
        u = rng.random(size=(m, read_len))
        sub = u < sub_rate
        alt = _ACGT[rng.integers(0, 4, size=(m, read_len), dtype=np.uint8)]
        r = np.where(sub, alt, r)
        isn = (u >= sub_rate) & (u < sub_rate + n_rate)
        r = np.where(isn, np.uint8(ord("N")), r)
        out[s:e] = r
    return out


def synth_two_haplotypes(n_reads: int, read_len: int, genome_len: int, seed: int, snp_every: int = 150,
                         sub_rate: float = 0.005, n_rate: float = 0.001) -> np.ndarray:
    """Very deep coverage of a small genome with two haplotypes (a substitution every `snp_every` bases): k-mer counters
    run into saturation, both alleles of a site reach the counter maximum (counts_level_t::mixed), the probabilistic
    counters work above their thresholds.  Same read model as synth_reads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
    b = a.copy()
    sites = np.arange(snp_every // 2, genome_len, snp_every)
    b[sites] = (b[sites] + 1 + rng.integers(0, 3, size=len(sites), dtype=np.uint8)) & 3
    hap = np.stack([_ACGT[a], _ACGT[b]])
    pos = rng.integers(0, genome_len - read_len + 1, size=n_reads, dtype=np.int64)
    which = rng.integers(0, 2, size=n_reads, dtype=np.int64)
    strand = rng.integers(0, 2, size=n_reads, dtype=np.uint8)
    ar = np.arange(read_len, dtype=np.int64)
    r = hap[which[:, None], pos[:, None] + ar[None, :]]
    r = np.where(strand[:, None] == 1, _COMP[r[:, ::-1]], r)
    u = rng.random(size=(n_reads, read_len))
    alt = _ACGT[rng.integers(0, 4, size=(n_reads, read_len), dtype=np.uint8)]
    r = np.where(u < sub_rate, alt, r)
    r = np.where((u >= sub_rate) & (u < sub_rate + n_rate), np.uint8(ord("N")), r)
    return np.ascontiguousarray(r)


def synth_quals(n_reads: int, read_len: int, seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed ^ 0x5EED))
    return _QUALS[rng.integers(0, len(_QUALS), size=(n_reads, read_len), dtype=np.uint8)]


def read_id(i: int, mate: int = 1) -> bytes:
    return b"@SRR000001.%d %d/%d" % (i + 1, i + 1, mate)


def synth_ids_varied(n: int, seed: int, mate: int = 0) -> list:
    """Illumina-style ids that exercise the id coder's branches: numeric fields with small / 2- / 3- / 4- / 8-byte
    positive and negative deltas, literal fields that change with and without a length change, 11+-digit digit
    runs (literal by rule), occasional format changes (token structure differs -> plain coding), several
    instrument names.  mate = 0: no mate suffix; 1 / 2: ' <mate>:N:0:<index>' (not 'typical' PE ids) -- every 7th
    pair instead ends in '/1' or '/2' (typical)."""
    rng = np.random.Generator(np.random.PCG64(seed ^ 0x1D5))
    instr = [b"@HWI-ST1234", b"@M00123", b"@NB501234", b"@A00987"]
    cells = [b"C0ABCACXX", b"H7LKJBGXY", b"000000000-AB12C", b"HW2YFDSXX"]
    out = []
    x = y = 1000
    big = 5_000_000_000
    for i in range(n):
        r = rng.integers(0, 1000)
        if r < 30:
            x = int(rng.integers(1, 30000)); y = int(rng.integers(1, 200000))
        elif r < 400:
            y += int(rng.integers(-1, 2))
        elif r < 800:
            y += int(rng.integers(-150, 300))
        else:
            y = int(rng.integers(1, 20_000_000))
        if r % 97 == 0:
            big = int(rng.integers(1, 9_999_999_999))
        elif r % 13 == 0:
            big += int(rng.integers(-70000, 70000))
        big = max(1, big)
        ins = instr[(i // 700) % 4 if r > 5 else int(rng.integers(0, 4))]
        cell = cells[(i // 1900) % 4]
        lane = 1 + (i // 500) % 8
        if r in (7, 8, 9):      # a different format altogether
            body = b"@read_%d length=%d" % (i, 100 + r)
        elif r in (10, 11):     # 11+ digits: literal by rule; separators only
            body = b"%s:%012d::%d" % (ins, big * 7, y)
        else:
            body = b"%s:%d:%s:%d:%d:%d:%d %d" % (ins, 100 + (i // 3000), cell, lane, 1101 + (i // 250) % 16, x, y, big)
        if mate:
            if i % 7 == 3:
                body += b"/%d" % mate
            else:
                body += b" %d:N:0:%s" % (mate, b"ATCACG" if (i // 1000) % 2 == 0 else b"TTAGGCA")
        out.append(body)
    return out


def synth_ids_zeros(n: int, seed: int) -> list:
    """Ids for the id *decoder*, which rebuilds a numeric field as decimal(previous value + delta) and so loses leading zeros:
    zero-padded numeric fields, fields whose digit count changes (9 -> 10, 100 -> 99), an 11-digit run (literal by rule, kept
    as it is) and empty tokens ('::')."""
    rng = np.random.Generator(np.random.PCG64(seed ^ 0x2E05))
    out = []
    a, b = 7, 100
    for i in range(n):
        a += 1                                   # 8, 9, 10, ...: the digit count grows
        b -= 1 if i % 3 == 0 else 0              # 100, 99, ...: and shrinks
        if b < 1:
            b = 120
        run = 10_000_000_000 + int(rng.integers(0, 89_999_999_999))   # 11 digits
        pad = int(rng.integers(0, 1000))
        if i % 41 == 17:
            out.append(b"@z%03d::%d::" % (pad, a))              # another shape: empty tokens next to the separators
        else:
            out.append(b"@zr.%03d:%d:%d::%011d:%05d/%02d" % (pad, a, b, run, i % 100000, 1 + i % 9))
    return out


def write_fastq(path: str, reads: np.ndarray, quals: np.ndarray | None = None,
                seed: int = 0, mate: int = 1) -> None:
    n, L = reads.shape
    if quals is None:
        quals = synth_quals(n, L, seed)
    with open(path, "wb") as f:
        buf = []
        for i in range(n):
            buf.append(read_id(i, mate))
            buf.append(b"\n")
            buf.append(reads[i].tobytes())
            buf.append(b"\n+\n")
            buf.append(quals[i].tobytes())
            buf.append(b"\n")
            if len(buf) >= 1 << 16:
                f.write(b"".join(buf))
                buf = []
        f.write(b"".join(buf))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    write_fastq(a.out, synth_reads(a.reads, a.len, a.genome, a.seed), seed=a.seed)


def synth_ragged(n_reads: int, genome_len: int, seed: int, min_len: int = 30, max_len: int = 160,
                 n_rate: float = 0.02, dup_rate: float = 0.05):
    """Variable-length reads with N runs and exact duplicates (edge cases of the DNA path).
    Returns (ids, seqs, quals) as lists of bytes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = _ACGT[rng.integers(0, 4, size=genome_len, dtype=np.uint8)]
    seqs = []
    for i in range(n_reads):
        if seqs and rng.random() < dup_rate:
            seqs.append(seqs[int(rng.integers(0, len(seqs)))])
            continue
        L = int(rng.integers(min_len, max_len + 1))
        pos = int(rng.integers(0, genome_len - L + 1))
        r = genome[pos:pos + L].copy()
        if rng.random() < 0.5:
            r = _COMP[r[::-1]]
        u = rng.random(L)
        r[u < 0.01] = _ACGT[rng.integers(0, 4, size=int((u < 0.01).sum()), dtype=np.uint8)]
        if rng.random() < 0.3:                      # an N run somewhere (possibly in the prefix)
            a = int(rng.integers(0, L))
            r[a:a + int(rng.integers(1, 6))] = ord("N")
        r[(u > 1.0 - n_rate)] = ord("N")
        seqs.append(r.tobytes())
    ids = [b"@rag.%d" % (i + 1) for i in range(n_reads)]
    quals = [bytes([33 + int(x) for x in rng.integers(2, 41, size=len(s))]) for s in seqs]
    return ids, seqs, quals


def synth_pairs(n_pairs: int, read_len: int, genome_len: int, seed: int, frag_min: int = 300, frag_max: int = 600,
                sub_rate: float = 0.005, n_rate: float = 0.001, chunk: int = 1 << 16):
    """Paired-end reads: fragment of random length, mate 1 from its start (forward), mate 2 the reverse
    complement of its end; fragment strand 50/50.  Returns two (n_pairs, read_len) uint8 arrays.
    The draws are, in this order: genome, fragment lengths, positions, strands, then per mate the (n, L) uniforms
    followed by the (n, L) substitution letters.  They are made in row chunks (memory: 5 M pairs need a few GB instead
    of tens) WITHOUT changing the stream: the uniforms of a mate come from a copy of the generator, the generator
    itself is advanced past them (one 64-bit step per double) and then supplies the letters; `chunk` is a multiple of
    8 rows so that every chunk of uint8 letters consumes whole 64-bit outputs."""
    assert chunk % 8 == 0
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = _ACGT[rng.integers(0, 4, size=genome_len, dtype=np.uint8)]
    frag = rng.integers(frag_min, frag_max + 1, size=n_pairs, dtype=np.int64)
    pos = (rng.random(n_pairs) * (genome_len - frag)).astype(np.int64)
    strand = rng.integers(0, 2, size=n_pairs, dtype=np.uint8)
    ar = np.arange(read_len, dtype=np.int64)
    out = []
    for mate in (0, 1):
        res = np.empty((n_pairs, read_len), dtype=np.uint8)
        bg_u = np.random.PCG64()
        bg_u.state = rng.bit_generator.state          # the uniforms: n * L doubles from here
        rng_u = np.random.Generator(bg_u)
        st0 = rng.bit_generator.state
        rng.bit_generator.advance(n_pairs * read_len)  # ... and the letters follow them
        st1 = rng.bit_generator.state                  # (advance() drops a cached 32-bit half, which the doubles would have left alone)
        st1["has_uint32"], st1["uinteger"] = st0["has_uint32"], st0["uinteger"]
        rng.bit_generator.state = st1
        for s in range(0, n_pairs, chunk):
            e = min(n_pairs, s + chunk)
            left = genome[pos[s:e, None] + ar[None, :]]
            right = _COMP[genome[(pos[s:e] + frag[s:e] - read_len)[:, None] + ar[None, :]][:, ::-1]]
            fwd = (strand[s:e, None] == 0) if mate == 0 else (strand[s:e, None] != 0)
            r = np.where(fwd, left, right)
            u = rng_u.random(size=(e - s, read_len))
            alt = _ACGT[rng.integers(0, 4, size=(e - s, read_len), dtype=np.uint8)]
            r = np.where(u < sub_rate, alt, r)
            res[s:e] = np.where((u >= sub_rate) & (u < sub_rate + n_rate), np.uint8(ord("N")), r)
        out.append(res)
    return out[0], out[1]


def synth_mixed_lengths(n_reads: int = 1500, genome_len: int = 40000, seed: int = 7):
    """Very short (20-31 bp, shorter than the b-mer), very long (4200-6000 bp, beyond the LDS staging
    buffer) and ordinary reads with N runs.  Returns (ids, seqs, quals) lists of bytes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = _ACGT[rng.integers(0, 4, size=genome_len, dtype=np.uint8)]
    ids, seqs, quals = [], [], []
    for i in range(n_reads):
        r = rng.random()
        L = int(rng.integers(20, 32)) if r < 0.4 else int(rng.integers(4200, 6000)) if r < 0.45 else int(rng.integers(60, 200))
        pos = int(rng.integers(0, genome_len - L))
        s = g[pos:pos + L].copy()
        if rng.random() < 0.3:
            s[int(rng.integers(0, L)):][:int(rng.integers(1, 12))] = ord("N")
        ids.append(b"@x%d" % i)
        seqs.append(s.tobytes())
        quals.append(b"I" * L)
    return ids, seqs, quals


def fastq_text(ids, seqs, quals, plus_id_every: int = 0, final_eol: bool = True) -> bytes:
    """FASTQ text of the records; plus_id_every = k > 0: every k-th record's separator line repeats the id (`+rag.7`);
    final_eol = False: the last line lacks its line feed."""
    out = []
    for i, (name, s, q) in enumerate(zip(ids, seqs, quals)):
        sep = b"+" + bytes(name)[1:] if plus_id_every and i % plus_id_every == 0 else b"+"
        out.append(bytes(name) + b"\n" + bytes(s) + b"\n" + sep + b"\n" + bytes(q) + b"\n")
    text = b"".join(out)
    return text if final_eol or not text else text[:-1]


def synth_c25_text() -> bytes:
    """2000 ragged reads, every third separator line carries the id, the text ends without a line feed (tests/golden/c25_*)"""
    return fastq_text(*synth_ragged(2000, 50000, 25), plus_id_every=3, final_eol=False)


# ---- c26: ids at the id kernel's staging limits and in the rare branches of the id coders (tests/golden/c26_*, tests/test_id_limits.py) ----
C26_DELTAS = [1, -1, 2, -2, 123, -123, 124, -124, 0xFFFF, -0xFFFF, 0x10000, -0x10000, 0xFFFFFF, -0xFFFFFF, 0x1000000, -0x1000000,
              0xFFFFFFFF, -0xFFFFFFFF, 0x100000000, -0x100000000]
_C26_SEPS = b",;+()~\t"   # separators that are none of " :._/-|=#"


def synth_ids_delta_walk(tag: bytes) -> list:
    """One numeric field that walks through every delta of C26_DELTAS -- both edges of every size class of the id coder's numeric
    deltas -- then from its value to 0, up to 9999999999 and back to 0 (the largest deltas ten digits allow), beside a field
    that counts up by one.  The values stay within ten digits and are never negative."""
    v, out = 5_000_000_000, []
    for k, d in enumerate([0] + C26_DELTAS + [None, 9_999_999_999, -9_999_999_999, 7]):
        v = 0 if d is None else v + d
        assert 0 <= v <= 9_999_999_999
        out.append(b"@%s.%d %d" % (tag, v, k + 1))
    return out


def synth_ids_at_limits() -> dict:
    """The ids of c26 that sit on the id kernel's staging limits ("in": the last value the kernel takes) or one beyond ("over")."""
    def many_tokens(n_sep, k):   # n_sep separators, so n_sep + 1 tokens with the line feed: literal and numeric tokens in turn
        return b"@t" + b"".join(bytes([_C26_SEPS[i % len(_C26_SEPS)]]) + (b"%d" % (i + k) if i % 2 else b"k%c" % (97 + (i + k) % 26)) for i in range(n_sep))

    def long_id(n, k):
        body = bytes(97 + (i * 7 + i // 26 + k * (i % 5 == 0)) % 26 for i in range(n - 8))
        return b"@long." + body + b".%d" % (k % 10)

    ids = {"in": [long_id(1023, 0), long_id(1023, 1), long_id(1023, 1), long_id(1022, 2)] + [many_tokens(127, k) for k in (0, 1, 1, 40)]
           + [b"@d.1234567890.12345678901", b"@d.1234567891.12345678902", b"@d.234567891.12345678902", b"@", b"@", b"@d.1.00000000002"],
           "over": [long_id(1024, 3), many_tokens(128, 5), long_id(1100, 4)]}
    assert [len(x) for x in ids["in"][:4]] == [1023, 1023, 1023, 1022] and [len(x) for x in ids["over"][::2]] == [1024, 1100]
    return ids


def synth_c26(name: str):
    """(ids, reads) of a single-end c26 input, (ids 1, reads 1, ids 2, reads 2) of the paired one; the reads are 60 bp
    (tools/make_golden.py --only c26 says how the reference coded each)."""
    rng = np.random.Generator(np.random.PCG64(0xC26))
    if name in ("ids_limits", "ids_over"):
        base, lim = synth_ids_varied(400, 26), synth_ids_at_limits()
        # (everything special twice: before the middle of the file and after it, so that with two workers each of them sees it)
        ids = base[:60] + synth_ids_delta_walk(b"walk") + base[60:120] + lim["in"] + base[120:200]
        ids += base[200:260] + lim["in"][::-1] + base[260:330] + synth_ids_delta_walk(b"w2")
        if name == "ids_over":
            ids += base[330:350] + lim["over"][:1] + base[350:360] + lim["over"][1:2] + base[360:380] + lim["over"][2:] + base[380:]
        else:
            ids += base[330:]
        return ids, synth_reads(len(ids), 60, 20000, 26)
    if name == "names":   # 3000 ids over 300 instrument names, one of them 62 bytes long, every seventh id on one of eight of the names
        names = [b"@%s%d%s" % ((b"HWI-ST", b"M0", b"NB50", b"A00_x", b"K")[j % 5], 1000 + 37 * j, b"" if j % 4 else b"-r%d" % (j % 7)) for j in range(300)]
        names[124] = b"@" + b"N62-" + bytes(65 + i % 26 for i in range(57))
        assert len(names[124]) == 62 and len(set(names)) == 300
        ids = []
        for i in range(3000):
            j = (i * 7919) % 300
            j = j % 8 if i % 7 == 0 else j
            ids.append(names[j] + (b".", b" ", b":")[i % 3] + b"%d %d/1" % (i + 1, i + 1))
        return ids, synth_reads(3000, 60, 20000, 27)
    if name == "names_over":   # 200 ids whose instrument names are 60 .. 64 bytes long
        ids = []
        for i in range(200):
            n = 60 + (i * 3 + i // 40) % 5
            nm = b"@" + (b"L%d-" % (i % 23)) + bytes(65 + (i % 23 + k) % 26 for k in range(64))
            ids.append(nm[:n] + (b":", b".", b" ")[i % 3] + b"%d:%d" % (1 + i // 50, 1000 + 13 * i))
        return ids, synth_reads(200, 60, 20000, 28)
    if name == "pe_long":   # 600 pairs, ids of 70 .. 200 bytes
        base = synth_ids_varied(600, 29)
        ids1, ids2 = [], []
        for i, x in enumerate(base):
            want = int(rng.integers(70, 199))
            x = x.replace(b" ", b"_") + b":"
            x = (x + bytes(45 if k % 20 == 19 else b"ACGT"[int(c)] for k, c in enumerate(rng.integers(0, 4, size=200))))[:max(want, 68) - 2]
            a, b = x + b"/1", x + b"/2"                       # i % 5 == 0: a typical pair
            if i % 5 == 1:                                     # the mates differ in one byte somewhere in 64 .. na - 3
                p = int(rng.integers(64, len(a) - 1))
                b = b[:p] + (b"Q" if b[p:p + 1] != b"Q" else b"R") + b[p + 1:]
            elif i % 5 == 2:                                   # ... at na - 3, the last byte idk_typical_pe compares
                b = x + b"_2"
            elif i % 5 == 3:                                   # the same id twice
                b = a
            elif i % 5 == 4:                                   # lengths that differ by one
                b = x + b"x/2"
            ids1.append(a)
            ids2.append(b)
        assert all(70 <= len(y) <= 200 for y in ids1 + ids2)
        return ids1, synth_reads(600, 60, 20000, 29), ids2, synth_reads(600, 60, 20000, 30)
    raise ValueError(name)


# name -> (fixture tag, paired, -om, -im, threads, every id within the id kernel's limits)
C26 = {"ids_limits": ("c26_ids_limits_o_t2", False, "o", "o", 2, True), "ids_over": ("c26_ids_over_o_t2", False, "o", "o", 2, False),
       "names": ("c26_names_s_i_t3", False, "s", "i", 3, True), "names_over": ("c26_names_over_o_i_t2", False, "o", "i", 2, False),
       "pe_long": ("c26_pe_long_o_o_t2", True, "o", "o", 2, True)}


# ---- c27: the quality encoder at its edges (tests/golden/c27_*, tests/test_quality.py, tests/test_fqs_file.py) ----
C27_WINDOW_LENS = [4031, 4032, 4033, 4095, 4096, 4097, 8063, 8064, 8065, 20, 63, 64, 65, 12100]


def _geometric(rng, n: int, k_max: int = 45) -> np.ndarray:
    """n draws of a geometric variable (p = 1/4, values 1 .. k_max + 1) from 32-bit integer draws: P(G > k) = (3/4)^k, the
    thresholds floor(2^32 (1 - (3/4)^k)) in integer arithmetic, so the values depend on no library's logarithm"""
    thr = np.array([(4 ** k - 3 ** k << 32) // 4 ** k for k in range(1, k_max + 1)], dtype=np.int64)
    return 1 + np.searchsorted(thr, rng.integers(0, 1 << 32, size=n, dtype=np.int64), side="right")


def _low_skewed_quals(rng, n: int) -> np.ndarray:
    """qualities 33 + min(G + 1, 41): 2 .. 41, the low ones frequent"""
    return (33 + np.minimum(_geometric(rng, n) + 1, 41)).astype(np.uint8)


def _split(flat: np.ndarray, lens) -> list:
    at = np.zeros(len(lens) + 1, dtype=np.int64)
    at[1:] = np.cumsum(lens)
    return [flat[at[i]:at[i + 1]].tobytes() for i in range(len(lens))]


def synth_c27(name: str):
    """(ids, seqs, quals), lists of bytes, of a c27 input (tools/make_golden.py --only c27 says how the reference coded each):
    "halving": 40 000 reads x 30 bp, low-skewed qualities -- coded by one worker, position 0's model passes 2^15;
    "windows": reads of C27_WINDOW_LENS x 3 -- both sides of the quality kernel's staging windows (4032 positions) and of its
               64-symbol chunks;
    "alphabet": 1200 reads of 20 .. 199 bp, quality symbols 0 .. 93 skewed to the top;
    "tiny_1" / "tiny_2" (40 reads) and "one_1" / "one_2" (1 read) of 20 .. 119 bp with synth_ids_varied ids: mate files of
               whole-file fixtures with far fewer reads than workers."""
    seed = {"halving": 271, "windows": 272, "alphabet": 273, "tiny_1": 274, "tiny_2": 275, "one_1": 276, "one_2": 277}[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    if name == "halving":
        lens = [30] * 40000
    elif name == "windows":
        lens = C27_WINDOW_LENS * 3
    elif name == "alphabet":
        lens = rng.integers(20, 200, size=1200).tolist()
    else:
        lens = rng.integers(20, 120, size=40 if name.startswith("tiny") else 1).tolist()
    total = int(sum(lens))
    seqs = _split(_ACGT[rng.integers(0, 4, size=total, dtype=np.uint8)], lens)
    if name == "alphabet":
        u = rng.integers(0, 100, size=total)
        sym = np.where(u < 15, rng.integers(0, 94, size=total), 93 - np.minimum(_geometric(rng, total) - 1, 93))
        assert sym.min() == 0 and sym.max() == 93
        quals = _split((33 + sym).astype(np.uint8), lens)
    else:
        quals = _split(_low_skewed_quals(rng, total), lens)
    if name[:-2] in ("tiny", "one"):
        ids = synth_ids_varied(len(lens), 27, int(name[-1]))   # (the mates of a pair share everything but the mate suffix)
    else:
        ids = [b"@c27.%d" % (i + 1) for i in range(len(lens))]
    return ids, seqs, quals


# quality-stream fixture -> (input, -qm, threads); all -s -om o -gs 1 -im n -qt 20
C27 = {}
for _qm in "o842":
    C27["c27_halving_%s_t1" % _qm] = ("halving", _qm, 1)
    C27["c27_alphabet_%s_t5" % _qm] = ("alphabet", _qm, 5)
for _qm in "o82":
    for _t in (1, 3):
        C27["c27_windows_%s_t%d" % (_qm, _t)] = ("windows", _qm, _t)
# whole-file fixture -> its inputs; all -om o -qm o -im o -gs 1 -t 64
C27_FILES = {"c27_tiny_se_o_oo_t64": ("tiny_1",), "c27_tiny_pe_o_oo_t64": ("tiny_1", "tiny_2"),
             "c27_one_se_o_oo_t64": ("one_1",), "c27_one_pe_o_oo_t64": ("one_1", "one_2")}
