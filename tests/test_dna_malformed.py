"""The DNA decoder (csrc/fqsx_dec.h, k_decode_{se,pe}_{orig,sorted}) on streams no encoder wrote, and on read offsets that do
not go with the streams.  It is the one decoder in which decoded symbols turn into memory indices: the p-mer search of a
sorted read's prefix (siv_select_equal), the anchor position and the candidate index of a second mate (pair_dec), and the k-mers
and pairs that decoded garbage sends into mailboxes and tables.

Nothing damaged is handed to a GPU.  The cases run on the emulation build through a stand-alone program
(tests/emu/dna_malformed_driver.cpp, with AddressSanitizer where the compiler has it) that also links the CPU oracle: a damaged
stream has to end in an error in both decoders or in the same bases in both, and a decoder that returns bases has to have learnt
what an encoder of these bases learns.  The points where a stream leaves the format are listed in DESIGN.md ("Where a DNA stream
leaves the format").

What this does not show: the emulation build is a 1-lane wave.  The bounds logic (fqsx_dec.h, the host's sizing in
block_prepare) is shared with the GPU build, the lane-parallel code around it (ballots, scans, the copies a wave makes) is not
exercised here."""
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import EMU_LIB, GOLD, ROOT, c1_records, c5_records, c20_records
from fqsqueezer_amd import hostpipe as hp
from test_dna_decode import MODES, _arrays, _cut

STREAMS, OFFSETS, REFUSED = 0, 1, 2   # a case's kind (dna_malformed_driver.cpp)


def _driver():
    """tests/emu/dna_malformed_driver.cpp linked with the emulation sources and the oracle: (program, sanitized).  With
    AddressSanitizer where the compiler has it; its runtime is linked statically, so the program needs nothing preloaded."""
    import __graft_entry__ as g
    bdir = os.path.join(ROOT, "build")
    os.makedirs(bdir, exist_ok=True)
    probe = subprocess.run(["g++", "-fsanitize=address", "-static-libasan", "-x", "c++", "-", "-o", os.path.join(bdir, "asan_probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    sanitized = probe.returncode == 0
    san = ["-fsanitize=address", "-static-libasan", "-fno-omit-frame-pointer"] if sanitized else []
    tag = "_asan" if sanitized else ""
    drv = os.path.join(ROOT, "tests", "emu", "dna_malformed_driver.cpp")
    osrc = [os.path.join(ROOT, "oracle", "fqs_oracle.cpp"), os.path.join(ROOT, "oracle", "fqs_oracle.h")]
    exe, oobj = os.path.join(bdir, "dna_malformed_driver" + tag), os.path.join(bdir, "fqs_oracle" + tag + ".o")
    if not g._newer(oobj, *osrc):   # the oracle with the flags of oracle/Makefile's `restate`
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off"] + san + ["-c", osrc[0], "-o", oobj])
    if not g._newer(exe, *(g._sources() + [drv, oobj])):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-DFQSX_EMU", "-ffp-contract=off", "-Wno-unused-function", "-pthread"] + san +
                              ["-x", "c++", drv, os.path.join(g.CSRC, "fqsx_api.hip"), os.path.join(g.CSRC, "fqsx_host.cpp"), "-x", "none", oobj, "-o", exe])
    return exe, sanitized


def _good_blocks(mode, which):
    """(header, [(bases, off)] x 3): the inputs of the cases"""
    paired = mode.startswith("pe")
    if which == "c20":   # 5000 bp mates: code lines and the reverse-complement line in scratch memory, not in LDS
        return hp.make_header(2, mode, 1), _cut(c20_records(), mode, [2, 2, 2])
    rec, header = (c5_records() if paired else c1_records()), hp.make_header(4, mode, 1)
    if mode.endswith("sorted"):   # the first three blocks of the file (one per bin of the sort)
        blks = (hp.form_blocks_pe(rec[0], rec[1], mode) if paired else hp.form_blocks(rec, mode))[:3]
        blocks = [_arrays(rec, mode, idx) for idx in blks]
    else:                         # (original order: form_blocks gives one block of the whole file)
        blocks = _cut(rec, mode, [40, 40, 40])
    if which == "few":            # fewer reads than workers in the last block
        bases, off = blocks[2]
        blocks[2] = (bases[:int(off[3])], off[:4])
    return header, blocks


def _with_reads(n_reads, T):
    return [t for t, (a, b) in enumerate(hp.partition_for_workers(n_reads, T)) if b > a]


def _stream_damage(streams, n_reads, T, rng, flips):
    """(label, streams) with one worker's stream damaged: cut to 1, 7, 8 bytes and to half; for every worker that has reads cut to
    0 bytes, every byte 0x00, every byte 0xFF (what a lost or blanked sector leaves); 1-3 flipped bytes (`flips` draws); every
    byte random; two workers' streams swapped"""
    ws, out = _with_reads(n_reads, T), []

    def put(label, w, s):
        out.append((label, streams[:w] + [bytes(s)] + streams[w + 1:]))
    for i, cut in enumerate((1, 7, 8, None)):
        w = ws[i % len(ws)]
        put("cut", w, streams[w][:len(streams[w]) // 2 if cut is None else cut])
    for w in ws:
        put("cut", w, b"")
        put("blank", w, bytes(len(streams[w])))
        put("blank", w, b"\xff" * len(streams[w]))
    for k in range(flips):
        w = ws[k % len(ws)]
        s = bytearray(streams[w])
        for _ in range(1 + k % 3):
            s[int(rng.integers(0, len(s)))] ^= int(rng.integers(1, 256))
        put("flip", w, s)
    w = ws[int(rng.integers(0, len(ws)))]
    put("random", w, rng.integers(0, 256, len(streams[w]), dtype=np.uint8).tobytes())
    if len(ws) > 1:
        s = list(streams)
        s[ws[0]], s[ws[-1]] = s[ws[-1]], s[ws[0]]
        out.append(("swap", s))
    return out


def _offset_damage(off, paired, rng):
    """(kind, off) with the streams intact: a length changed by +1 / -1 with the total kept, a length set to 0, the total grown
    by 1; refused: an offset that decreases, an odd number of reads in a paired mode"""
    n, out = len(off) - 1, []
    i = int(rng.integers(1, n - 1))
    for d in (1, -1):
        o = off.copy()
        o[i] = np.uint64(int(o[i]) + d)
        out.append((OFFSETS, o))
    o = off.copy()
    o[i + 1:] -= o[i + 1] - o[i]
    out.append((OFFSETS, o))
    o = off.copy()
    o[-1] += np.uint64(1)
    out.append((OFFSETS, o))
    o = off.copy()
    o[i], o[i + 1] = off[i + 1], off[i]
    assert o[i + 1] < o[i]
    out.append((REFUSED, o))
    if paired:
        out.append((REFUSED, off[:-1].copy()))
    return out


def _block_bytes(off, streams, bases=None):
    off = np.ascontiguousarray(off, dtype=np.uint64)
    out = [struct.pack("<I", len(off) - 1), off.tobytes()]
    if bases is not None:
        assert len(bases) == int(off[-1])
        out.append(np.ascontiguousarray(bases, dtype=np.uint8).tobytes())
    for s in streams:
        out += [struct.pack("<Q", len(s)), s]
    return b"".join(out)


def _groups():
    """the case file's groups: (mode, header, tiny, good blocks with their streams, [(kind, off, streams, label)])"""
    from fqsqueezer_amd.codec import DnaCodec
    groups, rng = [], np.random.default_rng(2024)
    for mode in MODES:
        paired = mode.startswith("pe")
        for which in ("file", "tiny", "c20" if paired else "few"):
            header, blocks = _good_blocks(mode, "file" if which == "tiny" else which)
            T = header[4]
            enc = DnaCodec(header, lib_path=EMU_LIB)
            streams = [enc.encode_block(bases, off, g) for g, (bases, off) in enumerate(blocks)]
            enc.close()
            off, n = blocks[2][1], len(blocks[2][1]) - 1
            cases = [(STREAMS, off, s, label) for label, s in _stream_damage(streams[2], n, T, rng, 20 if which in ("file", "tiny") else 8)]
            if which in ("file", "tiny"):
                cases += [(kind, o, streams[2], "offsets") for kind, o in _offset_damage(off, paired, rng)]
            groups.append((mode, header, which == "tiny", list(zip(blocks, streams)), cases))
    return groups


# Measured (AddressSanitizer build, all 428 cases, one core): the driver's run takes 330 s.  Nearly all of it is undamaged work --
# per case the two leading good blocks through the decoder and the oracle, after an error the three good blocks through a fresh
# codec, after bases two good blocks and the decoded one through an encoder, three to four codecs made and destroyed -- and a
# damaged block costs no more than a good one, so this is also what the same number of undamaged cases takes.  Limit: 10 x.
DRIVER_TIME_LIMIT = 3300

# How the stream-damage cases ended, errors / decoded, measured with the mix of _stream_damage over the three groups of a mode:
#                 all       cut      blank     flip     random   swap
#   se_original  28 / 68   9 / 13   19 / 1    0 / 48   0 / 3    0 / 3
#   se_sorted    44 / 52   6 / 16   12 / 8   22 / 26   2 / 1    2 / 1
#   pe_original  36 / 60   8 / 14   18 / 2    8 / 40   0 / 3    2 / 1
#   pe_sorted    41 / 55   4 / 18   12 / 8   21 / 27   2 / 1    2 / 1
# With the first mix (one worker cut to 0, 1, 7, 8 bytes and to half, 40 + 40 + 9 flips, one random stream, one swap) the
# original-order modes fell outside the floor: se_original 3 / 107, pe_original 19 / 91 (se_sorted 60 / 50, pe_sorted 35 / 75).
# A single-end read in original order has no point at which flipped bytes can leave the format -- letters and ranks decode from
# any bytes -- so no number of flips gets that mode to a quarter of errors: what does are streams that decode to the same read
# again and again ("Where a DNA stream leaves the format", point 3).  Hence every worker's stream is also cut to 0
# bytes and blanked with 0x00 and with 0xFF, and the flips are 20 + 20 + 8 a mode (48: the floor for them is 40).


def test_damaged_streams_and_offsets_end_in_an_error_or_inside_bounds(built, tmp_path, record_property):
    """Every case decodes two good blocks with a fresh codec and then the damaged third (T = 4, `-gs 1`: the first three blocks
    of c1 / c5, 40 reads or pairs a block in the original-order modes; once more with 64-slot tables at 85 % load, so that
    garbage k-mers walk overflow chains and post growths; paired modes: three blocks of 2 pairs of c20 at T = 2; single-end: a
    last block of 3 reads).  The driver requires what its header comment lists; here: it ends with code 0 inside the time limit,
    and in every mode at least a quarter of the stream-damage cases end in an error and at least a quarter in bases.
    The emulation build is a 1-lane wave: the bounds logic is the GPU build's, its lane-parallel code is not exercised."""
    groups = _groups()
    blob, n_cases, n_streams = [struct.pack("<I", len(groups))], 0, {m: 0 for m in range(4)}
    for mode, header, tiny, good, cases in groups:
        blob.append(bytes(header) + struct.pack("<II", int(tiny), len(good)))
        for (bases, off), streams in good:
            blob.append(_block_bytes(off, streams, bases))
        blob.append(struct.pack("<I", len(cases)))
        for kind, off, streams, _ in cases:
            blob.append(struct.pack("<I", kind) + _block_bytes(off, streams))
        n_cases += len(cases)
        n_streams[header[5]] += sum(c[0] == STREAMS for c in cases)
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    exe, sanitized = _driver()
    record_property("address_sanitizer", sanitized)
    print("damaged-DNA-stream driver:", exe, "(AddressSanitizer)" if sanitized else "(the compiler has no AddressSanitizer: plain build)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")   # (nothing is added to what the machine preloads)
    t0 = time.time()
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=DRIVER_TIME_LIMIT)
    record_property("driver_seconds", round(time.time() - t0, 1))
    print("the driver took %.1f s" % (time.time() - t0))
    print(r.stdout[-3000:])
    # how each kind of damage ended, per mode (what the comment above DRIVER_TIME_LIMIT records)
    table = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("CASE "):
            g, c, rc = int(ln.split()[1]), int(ln.split()[2]), int(ln.split(":")[1].split()[0])
            key = (groups[g][0], groups[g][4][c][3])
            table.setdefault(key, [0, 0])[0 if rc else 1] += 1
    for (mode, label), (n_err, n_ok) in sorted(table.items()):
        print(f"{mode:12s} {label:8s} {n_err:3d} errors {n_ok:3d} decoded")
    assert r.returncode == 0 and "DONE %d" % n_cases in r.stdout, f"sanitized={sanitized}\n" + r.stdout[-3000:] + r.stderr[-8000:]
    # a failed decode names the decode kernel
    text = [ln for ln in r.stdout.splitlines() if ln.startswith("TEXT ")]
    assert text and "device error 8 in decode kernel" in text[0], r.stdout[-3000:]
    split = {int(ln.split()[1]): (int(ln.split()[2]), int(ln.split()[3])) for ln in r.stdout.splitlines() if ln.startswith("SPLIT ")}
    for m, mode in enumerate(MODES):
        n_err, n_ok = split[m]
        record_property("split_" + mode, f"{n_err} errors / {n_ok} decoded")
        assert n_err + n_ok == n_streams[m] and sum(groups[g][4][c][3] == "flip" for g in range(len(groups)) if groups[g][0] == mode
                                                       for c in range(len(groups[g][4]))) >= 40
        assert 4 * n_err >= n_streams[m], f"{mode}: {n_err} of {n_streams[m]} damaged streams end in an error: under a quarter"
        assert 4 * n_ok >= n_streams[m], f"{mode}: {n_ok} of {n_streams[m]} damaged streams end in bases: under a quarter"


# ---- whole files ------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import os, resource, sys
sys.path.insert(0, sys.argv[1])
from fqsqueezer_amd import fqsread
from fqsqueezer_amd.codec import FqsxError
lib, good, out = sys.argv[2], sys.argv[3], sys.argv[4]
def run(path):
    try:
        fqsread.main(["d", path, "-out", out + ".1", "-out2", out + ".2", "-lib", lib])
    except (ValueError, FqsxError) as e:
        return type(e).__name__ + " " + str(e).replace("\n", " ")[:200]
    return "decoded"
print("GOOD", run(good), flush=True)
# the undamaged file's peak of address space, and 1 GiB for what threads and allocator arenas add from run to run: a decoder
# that sizes a buffer from a damaged length, not from the file's own read lengths, does not get it
peak = [int(ln.split()[1]) for ln in open("/proc/self/status") if ln.startswith("VmPeak:")][0] * 1024
resource.setrlimit(resource.RLIMIT_AS, (peak + (1 << 30), peak + (1 << 30)))
for path in sys.argv[5:]:
    print("CASE", os.path.basename(path), run(path), flush=True)
"""


def _damaged_files(name, tmp_path):
    """the first four blocks of a golden file as the good file, and four damaged versions of it"""
    header, blocks = hp.parse_fqs(open(os.path.join(GOLD, name), "rb").read())
    blocks, T, sids = blocks[:4], header[4], hp.stored_streams(header)
    chunks = list(hp.fqs_chunks(header, blocks))
    good = b"".join(chunks)
    start2 = sum(len(c) for c in chunks[:3])   # where block 2 starts
    files = {"good": good}
    # a. flipped bytes at the start of every worker's DNA stream of block 1
    bad = [hp.FqsBlock(b.n_reads, list(b.offsets), [dict(st) for st in b.streams]) for b in blocks]
    for w in range(T):
        s = bytearray(bad[1].streams[w][hp.STREAM_DNA])
        for i in range(min(4, len(s))):
            s[i] ^= 0xFF
        bad[1].streams[w][hp.STREAM_DNA] = bytes(s)
    files["flipped"] = hp.write_fqs(header, bad)
    # b. cut in the middle of block 2
    files["cut_in_block"] = good[:start2 + len(chunks[3]) // 2]
    # c. cut inside a stream-length varint: block 2 = varint(n_reads), varint(offset of worker 0), varint(length of its first stream)
    pos = start2
    for _ in range(2):
        _, pos = hp.get_varint(good, pos)
    files["cut_in_varint"] = good[:pos + 1]
    # d. the last stream of the last block: a length that points past the end of the file
    last = blocks[3].streams[T - 1][sids[-1]]
    at = len(good) - len(last) - len(hp.put_varint(len(last)))
    assert good[at:at + len(hp.put_varint(len(last)))] == hp.put_varint(len(last))
    files["length_past_the_end"] = good[:at] + hp.put_varint(0x3FFFFFFF) + good[at + len(hp.put_varint(len(last))):]
    paths = {}
    for k, v in files.items():
        paths[k] = tmp_path / (k + ".fqs")
        paths[k].write_bytes(v)
    return paths


@pytest.mark.parametrize("name", ["c1_10k_s_t4.fqs", "c5_pe4k_s_t4.fqs"])
def test_damaged_files_end_in_an_error(built, name, tmp_path):
    """A file with a damaged DNA stream, a file cut inside a block, a file cut inside a stream-length varint and a stream length
    that points past the end of the file, through `fqsread d` on the emulation library (no sanitizer) in a child process under
    a time limit: each ends in ValueError or FqsxError -- no crash, no hang -- and within the address space the undamaged file
    takes (+ 1 GiB), so nothing is sized from a damaged length.  The files are the first four blocks of the golden files;
    measured: the child takes 3-4 s."""
    paths = _damaged_files(name, tmp_path)
    cases = [k for k in paths if k != "good"]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, EMU_LIB, str(paths["good"]), str(tmp_path / "out")] + [str(paths[k]) for k in cases],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 1 + len(cases), r.stdout[-2000:] + r.stderr[-4000:]
    assert lines[0] == "GOOD decoded", lines[0]
    for k, ln in zip(cases, lines[1:]):
        assert ln.startswith(f"CASE {k}.fqs ValueError") or ln.startswith(f"CASE {k}.fqs FqsxError"), ln
    assert "decod" in lines[1] and "MemoryError" not in r.stdout, lines[1]
