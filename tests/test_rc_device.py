"""The device range coder and its exact division (csrc/fqsx_rc.h) on their own, through tests/emu/rc_driver.hip: a test-only
driver that this module compiles itself -- with hipcc for gfx950 (the `gpu` cases: hardware reciprocal + Newton step, 64
lanes, scalar coder state) and with g++ -DFQSX_EMU (the host cases: 1.0 / d, one lane) -- and loads with ctypes.

What is compared with what:
  division   div_u64_small / recip64_u16 for every divisor 1 .. 65535 (recip64_u16 from 2) against numpy's exact u64 floor
             division (itself spot-checked against Python integers): 65 535 x 468 operands.
  rc_step    one coding step from a set (low, range) against Encode (sub_rc.h:60-77) written in Python integers (_py_step),
             over every total 2 .. 2^15 + 96 and every range of the division set that is a coder state (>= 2^48).
  encoder    rc_open / rc_step / rc_end streams against the Python-integer encoder and the oracle's fqo_kat_rc, with
             buffers that are too small (the dropped-word rule) or fit exactly.
  decoder    rcd_start / rcd_cum / rcd_update over those streams against the Python-integer decoder, step by step.
Nothing here is compared with the project's own twin of the code under test."""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
MASK = (1 << 64) - 1
TOP = (1 << 48) - 1          # TopValue (sub_rc.h:38)
M56 = 0xFF << 56
U64, U32 = np.uint64, np.uint32


# ---- the driver ---------------------------------------------------------------------------------------------------------------
_libs = {}


def driver(where):
    if where in _libs:
        return _libs[where]
    import __graft_entry__ as g
    src = os.path.join(ROOT, "tests", "emu", "rc_driver.hip")
    out = os.path.join(ROOT, "tests", "emu", "rc_driver_%s.so" % where)
    if not g._newer(out, src, *g._sources()):
        tmp = out + ".tmp%d" % os.getpid()
        flags = ["-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unused-function"]
        if where == "gpu":
            cmd = ["hipcc", "--offload-arch=gfx950", "-O3"] + flags + [src, "-o", tmp]
        else:
            cmd = ["g++", "-O2", "-DFQSX_EMU"] + flags + ["-x", "c++", src, "-o", tmp]
        subprocess.check_call(cmd)
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.rcdrv_error.restype = C.c_char_p
    p, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.rcdrv_div.argtypes = [p, u32, p, u32, u32, u32, p, p]
    lib.rcdrv_step.argtypes = [u64, p, p, p, p, p, p, p]
    lib.rcdrv_encode.argtypes = [u32, p, p, p, p, p, u64, p, p, p, p]
    lib.rcdrv_decode.argtypes = [u32, p, p, p, p, p, u64, p, p, p]
    assert lib.rcdrv_is_gpu() == (where == "gpu")
    _libs[where] = lib
    return lib


def _ok(lib, rc):
    assert rc == 0, "rc_driver: %d %s" % (rc, lib.rcdrv_error().decode())


def _ptr(a):
    return a.ctypes.data


# ---- the operand set of the division --------------------------------------------------------------------------------------------
def _common_operands():
    xs = [((1 << b) + k) & MASK for b in range(64) for k in (-2, -1, 0, 1, 2)]
    xs += [MASK, MASK - 1, 0xff00000000000000, 1 << 56, (1 << 48) - 1]
    s = 88172645463325252
    for _ in range(64):   # xorshift64: the value and the value shifted down by its own low six bits
        s ^= (s << 13) & MASK
        s ^= s >> 7
        s ^= (s << 17) & MASK
        xs += [s, s >> (s & 63)]
    assert len(xs) == 320 + 5 + 128
    return np.array(xs, dtype=U64)


def _own_operands(d):
    """per divisor: the multiples of d nearest 2^64 - 1, 2^32 and 2^56, d * d and d << 32, each with its two neighbours (mod 2^64)"""
    d = d.astype(U64)
    top = (U64(MASK) // d) * d
    bases = [top, (U64(1 << 32) // d) * d, (U64(1 << 56) // d) * d, d * d, d << U64(32)]
    one = U64(1)
    return np.stack([b + k for b in bases for k in (U64(MASK), U64(0), one)], axis=1)   # (+ 2^64 - 1 = - 1)


_division_set = None


def division_set():
    """(d[65535], X[65535, 468], the 453 common operands)"""
    global _division_set
    if _division_set is None:
        d = np.arange(1, 65536, dtype=U64)
        xc = _common_operands()
        xp = np.ascontiguousarray(_own_operands(d))
        X = np.concatenate([np.broadcast_to(xc, (len(d), len(xc))), xp], axis=1)
        _division_set = (d, X, xc, xp)
    return _division_set


@pytest.mark.parametrize("where", WHERE)
def test_division_is_exact_for_every_divisor(where):
    """div_u64_small(x, d) == x // d and recip64_u16(d) == (2^64 - 1) // d for every d below 2^16, on powers of two and their
    neighbours, the top of the range, the multiples of d at the 2^32 seam between the two partial divisions, at 2^56 and at
    2^64 - 1, and xorshift values of every magnitude"""
    lib = driver(where)
    d, X, xc, xp = division_set()
    want = X // d[:, None]
    for i in range(0, X.size, 10007):   # numpy's u64 division is what the device is held against: it agrees with Python's
        r, c = divmod(i, X.shape[1])
        assert int(want[r, c]) == int(X[r, c]) // int(d[r])
    q = np.empty(X.shape, dtype=U64)
    recip = np.empty(len(d), dtype=U64)
    _ok(lib, lib.rcdrv_div(_ptr(xc), len(xc), _ptr(xp), xp.shape[1], 1, 65535, _ptr(q), _ptr(recip)))
    bad = np.argwhere(q != want)
    assert len(bad) == 0, "%d wrong quotients, the first: %s" % (len(bad), [(hex(int(X[r, c])), int(d[r]), int(q[r, c]), int(want[r, c])) for r, c in bad[:5]])
    want_recip = U64(MASK) // d
    bad = np.flatnonzero(recip[1:] != want_recip[1:]) + 1
    assert len(bad) == 0, "recip64_u16 wrong for d = %s" % [int(d[i]) for i in bad[:8]]


# ---- one coding step -------------------------------------------------------------------------------------------------------------
def _py_step(low, rng, freq, cum, tot):
    """Encode (sub_rc.h:60-77) in Python integers: (low, range, bytes written, carry-less branches taken), None if the
    renormalisation would not end (a range of 0)"""
    rng //= tot
    low = (low + rng * cum) & MASK
    rng *= freq
    out, n_cl = [], 0
    while rng <= TOP:
        if (low ^ ((low + rng) & MASK)) & M56:
            rng = ((low | TOP) - low) & MASK
            n_cl += 1
        if rng == 0 or len(out) == 16:
            return None
        out.append(low >> 56)
        low = (low << 8) & MASK
        rng = (rng << 8) & MASK
    return low, rng, bytes(out), n_cl


def _np_step(low, rng, freq, cum, tot):
    """_py_step on u64 arrays (u64 arithmetic wraps as the & MASK above): (low, range, len, bytes[n, 16], branch taken, ends)"""
    top, m56, eight = U64(TOP), U64(M56), U64(8)
    rng = rng // tot
    low = low + rng * cum
    rng = rng * freq
    n = len(low)
    out, ln, n_cl = np.zeros((n, 16), dtype=np.uint8), np.zeros(n, dtype=U64), np.zeros(n, dtype=bool)
    at = np.flatnonzero(rng <= top)   # the steps still renormalising, and their state
    lo, rg = low[at], rng[at]
    for it in range(17):
        if len(at) == 0:
            break
        cl = ((lo ^ (lo + rg)) & m56) != 0
        rg = np.where(cl, (lo | top) - lo, rg)
        n_cl[at[cl]] = True
        if it < 16:
            out[at, it] = (lo >> U64(56)).astype(np.uint8)
            ln[at] += U64(1)
            lo, rg = lo << eight, rg << eight
        low[at], rng[at] = lo, rg
        go = rg <= top
        at, lo, rg = at[go], lo[go], rg[go]
    return low, rng, ln, out, n_cl, rng > top


_step_cases = None


def step_cases():
    """Every total 2 .. 2^15 + 96 (the halving threshold plus the largest alphabet) x every operand of the division set that is a
    state of the coder (range >= 2^48; the multiples are those of the total).  Four (freq, cum) pairs -- the first, the last, a
    wide second and the whole interval of the model -- and four values of low make 16 combinations; pair (total t, range r) takes combination (t + r) mod 16, so that every total and every range
    meets all 16 while the set stays at 5.6 M steps (the division test, 30.7 M operands, is meant to be the largest part of this
    module; the full product would be 89 M steps).  Whether the quotient needs its fix-up depends on (range, total) alone, and
    every such pair is there.  Left out: the steps whose renormalisation never ends in the reference itself (low ends in 48 one
    bits when the carry-less branch is taken, so the new range is 0: no coder, reference or device, comes back from those), and
    those where a quotient one off would get there."""
    global _step_cases
    if _step_cases is None:
        _, _, xc, _ = division_set()
        tots = np.arange(2, (1 << 15) + 96 + 1, dtype=U64)
        own = _own_operands(tots)[:, [0, 1, 2, 6, 7, 8]]   # around the multiples nearest 2^64 - 1 and 2^56 (the others are below 2^48)
        R = np.concatenate([np.broadcast_to(xc[xc > U64(TOP)], (len(tots), int((xc > U64(TOP)).sum()))), own], axis=1)
        T = np.broadcast_to(tots[:, None], R.shape)
        combo = (np.arange(len(tots))[:, None] + np.arange(R.shape[1])[None, :]) % 16
        keep = R > U64(TOP)
        rng, tot, combo = R[keep], T[keep], combo[keep]
        lows = np.array([0, (1 << 56) - 1, 0x00ffffffffffff00, MASK >> 8], dtype=U64)
        low = lows[combo // 4]
        one = U64(1)
        freq = np.choose(combo % 4, [np.ones_like(tot), np.ones_like(tot), tot - one, tot])
        cum = np.choose(combo % 4, [np.zeros_like(tot), tot - one, np.ones_like(tot), np.zeros_like(tot)])
        ref = _np_step(low, rng, freq, cum, tot)
        # no way back from a range of 0: the carry-less branch taken while low ends in 48 one bits.  Such steps are left out for
        # the exact quotient and for a quotient one off, the error a broken multiply-high fix-up would make -- a defect there
        # has to fail this test, not leave a wave spinning
        risky, q = np.zeros(len(low), dtype=bool), rng // tot
        for dq in (U64(MASK), U64(0), U64(1)):
            l1, r1 = low + (q + dq) * cum, (q + dq) * freq   # (r1 == 0: (q + 1) * tot == 2^64)
            risky |= (r1 == U64(0)) | (((l1 & U64(TOP)) == U64(TOP)) & (r1 <= U64(TOP)))
        ends = ref[5]
        assert risky[~ends].all() and risky.sum() < len(ends) // 10
        keep = ~risky
        args = [np.ascontiguousarray(a[keep]) for a in (low, rng, freq, cum, tot)]
        _step_cases = (args, [a[keep] for a in ref[:5]], int(risky.sum()))
    return _step_cases


def test_step_reference_in_numpy_is_the_python_integer_one():
    """the vectorised reference the device is compared with, against Encode written out in Python integers: every 499th step
    and every seventh of the steps that take the carry-less branch"""
    (low, rng, freq, cum, tot), (rlow, rrng, rlen, rout, rcl), n_left_out = step_cases()
    assert len(low) > 5_000_000 and set(np.unique(tot)) == set(range(2, (1 << 15) + 97))
    assert rcl.sum() > 1000 and n_left_out < len(low) // 10
    for i in sorted(set(range(0, len(low), 499)) | set(np.flatnonzero(rcl)[::7].tolist())):
        got = _py_step(int(low[i]), int(rng[i]), int(freq[i]), int(cum[i]), int(tot[i]))
        assert got is not None and got[:2] == (int(rlow[i]), int(rrng[i])) and got[2] == rout[i, :int(rlen[i])].tobytes() and (got[3] > 0) == bool(rcl[i])
    # the steps left out are exactly those Python gives up on
    assert _py_step((1 << 56) - 1, 1 << 48, 1, 0, 2) is None


@pytest.mark.parametrize("where", WHERE)
def test_one_step_from_a_set_state(where):
    """low, range, length and bytes after one rc_step with a wave's lanes all on the same arguments: the multiply-high quotient
    with its low-32-bit fix-up, low + range * cum wrapping, the renormalisation and its carry-less branch"""
    lib = driver(where)
    (low, rng, freq, cum, tot), (rlow, rrng, rlen, rout, rcl), _ = step_cases()
    n = len(low)
    res, out = np.zeros((n, 3), dtype=U64), np.zeros((n, 16), dtype=np.uint8)
    f32, c32, t32 = (a.astype(U32) for a in (freq, cum, tot))
    _ok(lib, lib.rcdrv_step(n, _ptr(low), _ptr(rng), _ptr(f32), _ptr(c32), _ptr(t32), _ptr(res), _ptr(out)))
    bad = np.flatnonzero((res[:, 0] != rlow) | (res[:, 1] != rrng) | (res[:, 2] != rlen) | (out != rout).any(axis=1))
    assert len(bad) == 0, "%d wrong steps, the first (low, range, freq, cum, tot): %s" % (
        len(bad), [tuple(hex(int(a[i])) for a in (low, rng, freq, cum, tot)) for i in bad[:5]])


# ---- whole streams ---------------------------------------------------------------------------------------------------------------
def _py_encode(triples):
    """CRangeEncoder (sub_rc.h:34-86) in Python integers: (stream, carry-less branches taken)"""
    low, rng, out, n_cl = 0, M56, bytearray(), 0
    for freq, cum, tot in triples:
        got = _py_step(low, rng, freq, cum, tot)
        assert got is not None
        low, rng = got[:2]
        out += got[2]
        n_cl += got[3]
    for _ in range(8):   # End()
        out.append(low >> 56)
        low = (low << 8) & MASK
    return bytes(out), n_cl


def _py_decode(data, triples):
    """CRangeDecoder (sub_rc.h:93-158) in Python integers, bytes past the end read as 0: GetCumulativeFreq's value per step"""
    byte = lambda i: data[i] if i < len(data) else 0   # noqa: E731
    buf, pos = int.from_bytes(data[:8], "big"), 8
    low, rng, vals = 0, M56, []
    for freq, cum, tot in triples:
        rng //= tot
        vals.append(min(buf // rng, 0xffffffff))
        r = cum * rng
        buf -= r
        low = (low + r) & MASK
        rng *= freq
        while rng <= TOP:
            if (low ^ ((low + rng) & MASK)) & M56:
                rng = ((low | TOP) - low) & MASK
            buf = ((buf << 8) + byte(pos)) & MASK
            pos += 1
            low = (low << 8) & MASK
            rng = (rng << 8) & MASK
    return vals


def _table_script(rs, n, kmax, fmax):
    """n symbols, each from its own little model of 2 .. kmax symbols (the shape of test_range_coder_roundtrip): triples and
    per step (cumulative table, symbol)"""
    triples, tables = [], []
    for _ in range(n):
        k = int(rs.randint(2, kmax + 1))
        f = rs.randint(1, fmax, size=k)
        cums = [0] + np.cumsum(f).tolist()
        x = int(rs.choice(k, p=f / f.sum()))
        triples.append((cums[x + 1] - cums[x], cums[x], cums[-1]))
        tables.append((cums, x))
    return triples, tables


def _total_script(rs, tots):
    """one symbol per total: the first, the last or a random interval of the model"""
    triples = []
    for tot in tots:
        kind = int(rs.randint(0, 4))
        cum = 0 if kind == 0 else tot - 1 if kind == 1 else int(rs.randint(0, tot))
        freq = tot if kind == 0 and rs.randint(0, 8) == 0 else 1 if kind == 1 else int(rs.randint(1, tot - cum + 1))
        triples.append((freq, cum, tot))
    return triples


LONG_SYMBOLS = 120_000
LONG_CARRYLESS = 20   # the long script has to take the carry-less branch at least this often; it does LONG_MEASURED times


_scripts = None


def scripts():
    """[(name, triples, tables or None, reference stream, carry-less branches in the reference)]"""
    global _scripts
    if _scripts is None:
        rs = np.random.RandomState(3)
        out = []
        tr, tb = _table_script(rs, 5000, 5, 2000)
        out.append(("roundtrip-shape", tr, tb))
        edges = [2, 3, 4, 255, 256, 257, 65535 >> 1, (1 << 15) - 1, 1 << 15]
        out.append(("totals", _total_script(rs, list(range(2, 700)) + edges + rs.randint(2, (1 << 15) + 1, size=3000).tolist() + edges[::-1]), None))
        seen = set()
        for n in range(0, 400):   # short streams: the first 24, then whatever it takes for lengths of every value mod 8
            tr, tb = _table_script(rs, n % 50, 4, 300)
            r = len(_py_encode(tr)[0]) % 8
            if n < 24 or r not in seen:
                out.append(("short-%d" % n, tr, tb))
            seen.add(r)
        # long: skewed models with small totals (few bytes per symbol, the range mostly low) next to large ones
        tr = []
        for i in range(LONG_SYMBOLS):
            tot = int(rs.randint(2, 1 << 15)) if i % 3 else int(rs.randint(2, 40))
            cum = int(rs.randint(0, tot))
            tr.append((int(rs.randint(1, tot - cum + 1)), cum, tot))
        out.append(("long", tr, None))
        _scripts = [(name, tr, tb) + _py_encode(tr) for name, tr, tb in out]
    return _scripts


def _flat(all_triples):
    off = np.zeros(len(all_triples) + 1, dtype=U64)
    off[1:] = np.cumsum([len(t) for t in all_triples])
    flat = np.array([x for t in all_triples for x in t], dtype=U32).reshape(-1, 3)
    return off, [np.ascontiguousarray(flat[:, k]) for k in range(3)]


def _encode(lib, all_triples, caps, guard=256):
    """every script into its own stretch of one buffer filled with 0xA5: `guard` bytes, cap bytes for the stream, `guard` bytes.
    Returns per script (len, overflowed, the cap bytes, guards untouched)"""
    off, (freq, cum, tot) = _flat(all_triples)
    caps = np.array(caps, dtype=U64)
    out_off = np.zeros(len(caps), dtype=U64)
    at = 0
    for s, cap in enumerate(caps):
        out_off[s] = at + guard
        at += int(cap) + 2 * guard
    buf = np.full(at, 0xA5, dtype=np.uint8)
    lens, ovf = np.zeros(len(caps), dtype=U64), np.zeros(len(caps), dtype=U32)
    _ok(lib, lib.rcdrv_encode(len(caps), _ptr(off), _ptr(freq), _ptr(cum), _ptr(tot), _ptr(buf), len(buf), _ptr(out_off), _ptr(caps), _ptr(lens), _ptr(ovf)))
    res = []
    for s, cap in enumerate(caps):
        o, cap = int(out_off[s]), int(cap)
        clean = bool((buf[o - guard:o] == 0xA5).all() and (buf[o + cap:o + cap + guard] == 0xA5).all())
        res.append((int(lens[s]), bool(ovf[s]), buf[o:o + cap].tobytes(), clean))
    return res


def test_the_scripts_cover_what_they_are_for():
    """reference side only: stream lengths of every residue mod 8, totals from 2 to 2^15, and the long script takes the
    carry-less branch `range = (low | Top) - low` often enough"""
    sc = scripts()
    assert {len(s[3]) % 8 for s in sc} == set(range(8))
    tots = {t for _, tr, _, _, _ in sc for _, _, t in tr}
    assert min(tots) == 2 and max(tots) == 1 << 15
    name, tr, _, stream, n_cl = sc[-1]
    assert name == "long" and len(tr) >= 100_000 and n_cl >= LONG_CARRYLESS
    assert n_cl == LONG_MEASURED, n_cl


LONG_MEASURED = 53   # carry-less branches the Python reference takes in the long script (measured; asserted above)


@pytest.mark.parametrize("where", WHERE)
def test_encoder_streams(where):
    """rc_open / rc_step / rc_end, one workgroup per script, into buffers with room: the bytes of the Python-integer encoder and
    of the oracle's fqo_kat_rc.  The long script (120 000 symbols) takes the carry-less branch 53 times in the
    reference (LONG_MEASURED)."""
    from oracle.pyoracle import lib as olib
    lib, sc = driver(where), scripts()
    for name, tr, _, stream, _ in sc:
        _, (freq, cum, tot) = _flat([tr])
        out = np.zeros(len(stream) + 64, dtype=np.uint8)
        ln = olib().fqo_kat_rc(len(tr), _ptr(freq), _ptr(cum), _ptr(tot), _ptr(out), len(out))
        assert out[:ln].tobytes() == stream, "the oracle's stream differs from the Python encoder's: " + name
    caps = [(len(s[3]) + 7) // 8 * 8 + 8 for s in sc]
    for (name, _, _, stream, _), (ln, ovf, data, clean) in zip(sc, _encode(lib, [s[1] for s in sc], caps)):
        assert ln == len(stream) and not ovf and clean, name
        assert data[:ln] == stream, name + ": stream differs at byte %d" % next(i for i in range(ln) if data[i] != stream[i])


@pytest.mark.parametrize("where", WHERE)
def test_encoder_output_buffer_too_small_or_exact(where):
    """the dropped-word rule: with cap < length (cap a multiple of 8, 0 included) len goes on counting to the reference's
    length, rc_overflowed says so, the first cap bytes are the reference's and nothing beyond cap is written; with cap == length
    (a length that is a multiple of 8) the stream is complete and has not overflowed"""
    lib, sc = driver(where), scripts()
    cases = []
    for name, tr, _, stream, _ in sc[:-1]:
        n8 = len(stream) // 8 * 8
        for cap in sorted({0, 8, n8 - 8, n8 if n8 < len(stream) else n8 - 8, n8 // 2 // 8 * 8}):
            if 0 <= cap < len(stream):
                cases.append((name, tr, stream, cap))
        if len(stream) % 8 == 0:
            cases.append((name, tr, stream, len(stream)))
    assert sum(1 for c in cases if c[3] == len(c[2])) >= 2 and sum(1 for c in cases if c[3] == 0) >= 8
    for (name, _, stream, cap), (ln, ovf, data, clean) in zip(cases, _encode(lib, [c[1] for c in cases], [c[3] for c in cases])):
        what = "%s cap %d of %d" % (name, cap, len(stream))
        assert ln == len(stream), what
        assert ovf == (cap < len(stream)), what
        assert data == stream[:cap], what
        assert clean, what + ": bytes outside the stream's buffer were written"


@pytest.mark.parametrize("where", WHERE)
def test_decoder_follows_the_streams(where):
    """rcd_start / rcd_cum / rcd_update over the reference streams with a plain byte source (bytes past the end read as 0):
    rcd_cum's value at every step is the Python decoder's, and it names the script's symbol"""
    lib, sc = driver(where), scripts()
    off, (freq, cum, tot) = _flat([s[1] for s in sc])
    streams = np.frombuffer(b"".join(s[3] for s in sc), dtype=np.uint8)
    st_len = np.array([len(s[3]) for s in sc], dtype=U64)
    st_off = np.zeros(len(sc), dtype=U64)
    st_off[1:] = np.cumsum(st_len)[:-1]
    got = np.zeros(int(off[-1]), dtype=U32)
    _ok(lib, lib.rcdrv_decode(len(sc), _ptr(off), _ptr(freq), _ptr(cum), _ptr(tot), _ptr(streams), len(streams), _ptr(st_off), _ptr(st_len), _ptr(got)))
    for s, (name, tr, tables, stream, _) in enumerate(sc):
        g = got[int(off[s]):int(off[s + 1])].tolist()
        want = _py_decode(stream, tr)
        assert g == want, name + ": rcd_cum differs from the Python decoder at step %d" % next(i for i in range(len(g)) if g[i] != want[i])
        assert all(c <= v < c + f for v, (f, c, _) in zip(g, tr)), name
        if tables:
            assert [bisect.bisect_right(cums, v) - 1 for v, (cums, _) in zip(g, tables)] == [x for _, x in tables], name
