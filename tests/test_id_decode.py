"""The id stream decoders: k_id_decode (csrc/fqsx_iddec.h, fqsx_idg_decode_block) against its host twin
(fqsx_id_decode_block) and against a statement, in Python, of what the reference's `fqs d` writes for an id -- which is not
always the id its encoder was given (store_int, id.h:117-149; instrument mode; the mate-2 copy of typical pairs).  The
whole-file side is in test_fqs_fastq.py.  Emulation build and, marked gpu, device 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import EMU_LIB, ROOT
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import FqsxError, IdCodec
from test_id_gpu import CASES, _arrays, _ids

WHERE = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


# ---- the reference's output rules ------------------------------------------------------------------------------------------------
def _is_lit(c):
    return 48 <= c <= 57 or 65 <= c <= 90 or 97 <= c <= 122 or c == 64   # id.cpp:57-70


def _tokens(line: bytes):
    """tokenize, id.cpp:734-757: (numeric, separator, text) per token; a token ends at every byte that is not a literal one"""
    out, start = [], 0
    for i, c in enumerate(line):
        if not _is_lit(c):
            t = line[start:i]
            out.append((t.isdigit() and 1 <= len(t) <= 10, c, t))
            start = i + 1
    return out


class RefWorker:
    """One worker's view: what decompress_lossless / decompress_instrument give back for the lines compress_* was given."""

    def __init__(self, mode):
        self.mode, self.names = mode, {}   # instrument mode: name as given -> name as decoded (the move-to-front lists persist)
        self.reset()

    def reset(self):   # ResetReadPrev, once per block
        self.prev = None

    def lossless(self, line: bytes) -> bytes:
        cur = _tokens(line)
        same = self.prev is not None and len(cur) == len(self.prev) and all(a[:2] == b[:2] for a, b in zip(cur, self.prev))
        self.prev = cur
        if not same:
            return line   # the plain path: byte for byte
        # the same-types path: a numeric token comes back as store_int(previous value + delta) = the decimal form of its value
        return b"".join((b"%d" % int(t) if num else t) + bytes([sep]) for num, sep, t in cur)

    def instrument(self, line: bytes) -> bytes:
        n = min(i for i, c in enumerate(line) if c in b". :")
        name = line[:n]
        if name not in self.names:   # through the lossless path with its terminating 0; the 0 becomes the line feed
            self.names[name] = self.lossless(name + b"\0")[:-1]
        return self.names[name] + b"\n"


class RefModel:
    def __init__(self, T, mode, paired):
        self.T, self.mode, self.paired = T, mode, paired
        self.w = [RefWorker(mode) for _ in range(T)]

    def block(self, lines):
        out = []
        for t, (first, last) in enumerate(hp.partition_for_workers(len(lines), self.T)):
            w = self.w[t]
            w.reset()
            one = w.lossless if self.mode == "lossless" else w.instrument
            step = 2 if self.paired else 1
            for i in range(first, last, step):
                if not self.paired or self.mode != "lossless":
                    out += [one(x) for x in lines[i:i + step]]
                    continue
                a, b = lines[i], lines[i + 1]
                typical = len(a) == len(b) and len(a) >= 3 and a[:-2] == b[:-2] and a[-2:-1] == b"1" and b[-2:-1] == b"2"   # id.cpp:241-254
                o1 = one(a)
                out += [o1, o1[:-2] + b"2" + o1[-1:]] if typical else [o1, one(b)]
        return out


def _case_ids(kind, n, paired):
    ids = _ids(kind, n, 5)
    if paired:   # mates: mostly the typical .../1 .../2 pair, sometimes not (as test_id_gpu._compare)
        both = []
        for i, x in enumerate(ids):
            both.append(x + b"/1")
            both.append((x if i % 11 else x[:-1] + b"Z") + b"/2")
        ids = both
    return ids


def _lines_of(ids, off):
    b = bytes(ids)
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def _round_trip(lib, T, id_mode, kind, paired, n, blocks):
    header = hp.make_header(T, "pe_sorted" if paired else "se_sorted", 1, id_mode=id_mode)
    enc_h, enc_g = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    dec_h, dec_g = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    cross_h, cross_g = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)   # the directions crossed
    model = RefModel(T, id_mode, paired)
    ids = _case_ids(kind, n, paired)
    per = len(ids) // blocks // 2 * 2
    changed = 0
    for b in range(blocks):
        lines = [x + b"\n" for x in ids[b * per:(b + 1) * per]]
        a, off = _arrays(ids[b * per:(b + 1) * per])
        st_h, st_g = enc_h.encode_block(a, off, paired), enc_g.encode_block(a, off, paired)
        want = model.block(lines)
        h_ids, h_off = dec_h.decode_block(st_g, per, paired)
        g_ids, g_off = dec_g.decode_block(st_g, per, paired)
        assert np.array_equal(g_off, h_off) and np.array_equal(g_ids, h_ids), f"block {b}: the GPU decoder differs from the host decoder"
        assert _lines_of(h_ids, h_off) == want, f"block {b}: the decoders differ from the reference's output rules"
        x_ids, x_off = cross_g.decode_block(st_h, per, paired)       # host-encoded streams through the GPU decoder
        assert np.array_equal(x_off, h_off) and np.array_equal(x_ids, h_ids), f"block {b}: host-encoded streams through the GPU decoder"
        x_ids, x_off = cross_h.decode_block(st_g, per, paired)       # GPU-encoded streams through the host decoder
        assert np.array_equal(x_off, h_off) and np.array_equal(x_ids, h_ids), f"block {b}: GPU-encoded streams through the host decoder"
        assert np.array_equal(dec_g.state(), enc_g.state()), f"block {b}: the decoder's state words differ from the encoder's"
        changed += sum(x != y for x, y in zip(want, lines))
    for c in (enc_h, enc_g, dec_h, dec_g, cross_h, cross_g):
        c.close()
    return changed


@pytest.mark.parametrize("T,id_mode,kind,paired", CASES)
def test_emu_id_decoder_round_trip(built, T, id_mode, kind, paired):
    changed = _round_trip(EMU_LIB, T, id_mode, kind, paired, n=1200, blocks=3)
    if id_mode == "instrument" or kind == "illumina":   # (the flow cell "000000000-A1B2C": a numeric token of nine zeros)
        assert changed > 0


@pytest.mark.gpu
@pytest.mark.parametrize("T,id_mode,kind,paired", CASES + [(64, "lossless", "illumina", False), (64, "instrument", "illumina", True),
                                                           (1, "lossless", "illumina", True), (255, "lossless", "odd", False)])
def test_gpu_id_decoder_round_trip(T, id_mode, kind, paired):
    _round_trip(None, T, id_mode, kind, paired, n=20000, blocks=5)


def test_reference_rules_model_normalises_numeric_fields():
    """the Python statement above, on its own: leading zeros go only on the same-types path"""
    w = RefWorker("lossless")
    assert w.lossless(b"@a.007:x\n") == b"@a.007:x\n"            # first line: plain
    assert w.lossless(b"@a.008:x\n") == b"@a.8:x\n"              # same token types: store_int
    assert w.lossless(b"@a.00000000009:x\n") == b"@a.00000000009:x\n"   # 11 digits: a literal token, other types: plain
    assert w.lossless(b"@a.00000000010:x\n") == b"@a.00000000010:x\n"   # literal again, same types: kept as it is


# ---- re-sizing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
def test_decoder_grows_from_tiny_capacities(where, request, monkeypatch):
    lib = None
    if where == "emu":
        request.getfixturevalue("built")
        lib = EMU_LIB
    header = hp.make_header(3, "se_sorted", 1, id_mode="lossless")
    enc, ref = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib)
    monkeypatch.setenv("FQSX_IDG_INIT", "1")
    dec = IdCodec(header, lib_path=lib, device=0)
    monkeypatch.delenv("FQSX_IDG_INIT")
    s0 = dec.stats()
    assert s0["small_slots"] == 16 and s0["big_slots"] == 16
    ids = _ids("illumina", 3000, 7)
    for b in range(3):
        a, off = _arrays(ids[b * 1000:(b + 1) * 1000])
        st = enc.encode_block(a, off)
        want, got = ref.decode_block(st, 1000), dec.decode_block(st, 1000)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"block {b}"
    s = dec.stats()
    assert s["retries"] >= 3 and s["grow_small"] >= 1 and s["grow_big"] >= 1 and s["grow_out"] >= 1, s
    assert s["out_bytes"] > 64


# ---- malformed streams (emulation build only: nothing that might fault a shared GPU is run there on purpose) --------------------
def _malformed_cases():
    """(header, n_reads, paired, streams) with streams cut to 0, 7 and half their bytes and with flipped bytes"""
    out = []
    for id_mode, kind, paired in (("lossless", "illumina", False), ("lossless", "odd", True), ("instrument", "illumina", False)):
        header = hp.make_header(2, "pe_sorted" if paired else "se_sorted", 1, id_mode=id_mode)
        ids = _ids(kind, 600, 3)
        if paired:
            ids = [y for i, x in enumerate(ids[:300]) for y in (x + b"/1", (x if i % 5 else x + b"q") + b"/2")]
        a, off = _arrays(ids)
        st = IdCodec(header, lib_path=EMU_LIB).encode_block(a, off, paired)
        bad = [[st[0][:0], st[1]], [st[0][:7], st[1]], [st[0], st[1][:7]], [st[0], st[1][:len(st[1]) // 2]], [st[0][:len(st[0]) // 2], st[1]]]
        rng = np.random.default_rng(11)
        for k in range(40):
            s = [bytearray(x) for x in st]
            for _ in range(1 + k % 4):
                w = int(rng.integers(0, 2))
                s[w][int(rng.integers(0, len(s[w])))] ^= int(rng.integers(1, 256))
            bad.append([bytes(x) for x in s])
        out += [(header, len(ids), paired, b) for b in bad]
    return out


def _malformed_driver():
    """tests/emu/id_malformed_driver.cpp linked with the emulation sources: (program, sanitized).  With AddressSanitizer where
    the compiler has it (host code); its runtime is linked statically, so the program needs nothing preloaded."""
    import __graft_entry__ as g
    bdir = os.path.join(ROOT, "build")
    os.makedirs(bdir, exist_ok=True)
    src = [os.path.join(ROOT, "tests", "emu", "id_malformed_driver.cpp"), os.path.join(g.CSRC, "fqsx_api.hip"), os.path.join(g.CSRC, "fqsx_host.cpp")]
    base = ["g++", "-O1", "-g", "-std=c++17", "-DFQSX_EMU", "-ffp-contract=off", "-Wno-unused-function", "-pthread", "-x", "c++"] + src
    probe = subprocess.run(["g++", "-fsanitize=address", "-static-libasan", "-x", "c++", "-", "-o", os.path.join(bdir, "asan_probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    sanitized = probe.returncode == 0
    exe = os.path.join(bdir, "id_malformed_driver_asan" if sanitized else "id_malformed_driver")
    if not g._newer(exe, *(g._sources() + src[:1])):
        subprocess.check_call(base + (["-fsanitize=address", "-static-libasan", "-fno-omit-frame-pointer"] if sanitized else []) + ["-o", exe])
    return exe, sanitized


def test_malformed_streams_end_in_an_error_or_inside_bounds(built, tmp_path, record_property):
    import struct
    cases = _malformed_cases()
    blob = [struct.pack("<I", len(cases))]
    for header, n, paired, streams in cases:
        blob.append(bytes(header) + struct.pack("<III", n, int(paired), len(streams)))
        for x in streams:
            blob.append(struct.pack("<Q", len(x)) + x)
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    exe, sanitized = _malformed_driver()
    record_property("address_sanitizer", sanitized)
    print("malformed-stream driver:", exe, "(AddressSanitizer)" if sanitized else "(the compiler has no AddressSanitizer: plain build)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=900)   # every call returns within the time limit
    assert r.returncode == 0 and "DONE" in r.stdout, f"sanitized={sanitized}\n" + r.stdout[-2000:] + r.stderr[-6000:]
    n_err, n_ok, n_short = (int(x) for x in r.stdout.split("DONE")[1].split()[:3])
    assert n_err + n_ok + n_short == 2 * len(cases)
    assert n_short == 2 * 3 * 3, "streams under 8 bytes of a worker with reads: FQSX_E_ARG from both decoders"
    assert n_err > 0


def test_stream_under_8_bytes_is_a_bad_argument(built):
    header = hp.make_header(2, "se_sorted", 1, id_mode="lossless")
    a, off = _arrays(_ids("srr", 100, 1))
    st = IdCodec(header, lib_path=EMU_LIB).encode_block(a, off)
    for device in (None, 0):
        for cut in (0, 7):
            with pytest.raises(FqsxError, match=": -1:"):
                IdCodec(header, lib_path=EMU_LIB, device=device).decode_block([st[0][:cut], st[1]], 100)


# ---- the models across a halving ---------------------------------------------------------------------------------------------------
def _halving_ids(n):
    """one numeric field whose delta stays in 4..7: every id decodes symbol 3 of the same 4-symbol model and one symbol of the same
    256-symbol model, so both totals reach 2^15 and are halved (rc.h:41-55) inside one worker"""
    v, out = 0, []
    for i in range(n):
        v += 4 + i % 4
        out.append(b"@h.%d" % v)
    return out


def _halving(lib, n=40000, blocks=2):
    header = hp.make_header(1, "se_sorted", 1, id_mode="lossless")
    enc_h, enc_g = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    dec_h, dec_g = IdCodec(header, lib_path=lib), IdCodec(header, lib_path=lib, device=0)
    ids = _halving_ids(n)
    per = n // blocks
    for b in range(blocks):
        a, off = _arrays(ids[b * per:(b + 1) * per])
        st = enc_g.encode_block(a, off)
        assert st == enc_h.encode_block(a, off)
        for dec in (dec_h, dec_g):
            got, got_off = dec.decode_block(st, per)
            assert np.array_equal(got_off, off) and np.array_equal(got, a), f"block {b}"   # (no leading zeros: the ids come back as given)
        assert np.array_equal(dec_g.state(), enc_g.state())


def test_emu_models_agree_across_a_halving(built):
    _halving(EMU_LIB)


@pytest.mark.gpu
def test_gpu_models_agree_across_a_halving():
    _halving(None)
