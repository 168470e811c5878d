"""Rate of the quality decoder (k_qual_decode) against the DNA decoder on reads of the same shape, in one run.
Input: the benchmark's shape, n x 150 symbols of synth_quals, T = 64, -qm o and -qm 8.  Every quality block is encoded once,
then all blocks are decoded through a fresh decoder per pass: a warm-up pass, then `reps` passes alternating with the
yardstick, the DNA decoder (fqsx_dna_decode_block) on n x 150 bases.  Kernel time: HIP events (fqsx_qual_kernel_times /
fqsx_dna_kernel_times, a pass of its own for the DNA decoder because timing waits for every launch); wall clock: around the
decode calls of a pass, transfers included.  Gate: quality symbols/s >= DNA bases/s, wall against wall and kernel against
kernel, medians.  Writes profiles/qual_decode.json.
usage: python tools/gpu_qual_decode.py [--reads 1000000] [--reps 3] [--alt-lib build-with-FQSX_QDEC_NO_LOOKAHEAD.so] [--out file]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DnaCodec, QualCodec
from fqsqueezer_amd.synth import read_id, synth_quals, synth_reads

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--alt-lib", default=None, help="a diagnostic build with -DFQSX_QDEC_NO_LOOKAHEAD, timed beside the product library")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qual_decode.json"))
a = ap.parse_args()
n, L, T = a.reads, 150, 64
genome = max(1000000, n * L // 20)
reads = synth_reads(n, L, genome, 2)
rec = hp.Records([read_id(i) for i in range(n)], reads, synth_quals(n, L, 2))
blks = hp.form_blocks(rec, "se_sorted")
n_sym = n * L


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v), "all": [round(x, 3) for x in v]}


# ---- the yardstick: the DNA decoder on the same reads
dna_header = hp.make_header(T, "se_sorted", max(1, genome // 1000000))
dna_blocks = [hp.block_arrays(rec, idx) for idx in blks]
enc = DnaCodec(dna_header)
dna_streams = [enc.encode_block(b, o, g) for g, (b, o) in enumerate(dna_blocks)]
enc.close()


def dna_pass(profiled):
    dec = DnaCodec(dna_header)
    dec.set_profiling(profiled)
    ok, t0 = True, time.perf_counter()
    outs = [dec.decode_block(dna_streams[g], o, g) for g, (b, o) in enumerate(dna_blocks)]
    wall = time.perf_counter() - t0
    kt = dec.kernel_times()
    dec.close()
    for out, (b, o) in zip(outs, dna_blocks):
        ok = ok and bool(np.array_equal(out, np.asarray(b)))
    assert ok, "DNA round trip failed"
    return wall, (kt["encode_ms"] + kt["insert_ms"] + kt["other_ms"]) / 1e3


def qual_pass(header, arrs, streams, lib):
    dec = QualCodec(header, lib_path=lib)
    dec.set_profiling(True)
    t0 = time.perf_counter()
    outs = [dec.decode_block(st, off) for st, (q, off) in zip(streams, arrs)]
    wall = time.perf_counter() - t0
    ms = dec.kernel_times()["encode_ms"]
    dec.close()
    for out, (q, off) in zip(outs, arrs):
        assert np.array_equal(out, header_want(header, q)), "quality round trip failed"
    return wall, ms / 1e3


REV8 = np.array([0, 6, 15, 22, 27, 33, 37, 40], dtype=np.uint8)   # quality.cpp:84-117
FWD8 = np.array([0] * 2 + [1] * 8 + [2] * 10 + [3] * 5 + [4] * 5 + [5] * 5 + [6] * 5 + [7] * 56, dtype=np.uint8)


def header_want(header, q):
    return q if header[6] == 0 else (REV8[FWD8[q - 33]] + 33).astype(np.uint8)


res = {"device": "MI355X (gfx950)", "reads": n, "read_len": L, "T": T, "blocks": len(blks), "reps": a.reps, "modes": {}}
modes = {"lossless": {}, "illumina_8": {}}
for qm, m in modes.items():
    m["header"] = hp.make_header(T, "se_sorted", 5, qm, "none")
    m["arrs"] = [hp.qual_arrays(rec, idx) for idx in blks]
    e = QualCodec(m["header"])
    e.set_profiling(True)
    m["streams"] = [e.encode_block(q, off) for q, off in m["arrs"]]
    m["enc_s"] = e.kernel_times()["encode_ms"] / 1e3
    m["contexts"] = sum(e.contexts()["per_worker"])
    e.close()
    m["wall"], m["kern"], m["alt_wall"], m["alt_kern"] = [], [], [], []

# warm-up pass of everything, then the passes alternate
dna_pass(False)
for m in modes.values():
    qual_pass(m["header"], m["arrs"], m["streams"], None)
dna_wall, dna_kern = [], []
for rep in range(a.reps):
    dna_wall.append(dna_pass(False)[0])
    for m in modes.values():
        w, k = qual_pass(m["header"], m["arrs"], m["streams"], None)
        m["wall"].append(w); m["kern"].append(k)
    dna_kern.append(dna_pass(True)[1])
    if a.alt_lib:
        for m in modes.values():
            w, k = qual_pass(m["header"], m["arrs"], m["streams"], os.path.abspath(a.alt_lib))
            m["alt_wall"].append(w); m["alt_kern"].append(k)

rate = lambda secs: [n_sym / s / 1e6 for s in secs]   # noqa: E731
res["dna_decode_mbases_s"] = {"wall": spread(rate(dna_wall)), "kernel": spread(rate(dna_kern)),
                              "earlier_rounds_DESIGN_md": "9.4-10.3 Mbases/s (not the yardstick)"}
gate = True
for qm, m in modes.items():
    r = {"decode_msymbols_s": {"wall": spread(rate(m["wall"])), "kernel": spread(rate(m["kern"]))},
         "encode_kernel_msymbols_s": round(n_sym / m["enc_s"] / 1e6, 3), "contexts": m["contexts"],
         "bits_per_symbol": round(8 * sum(len(s) for st in m["streams"] for s in st) / n_sym, 4)}
    if a.alt_lib:
        r["decode_msymbols_s_without_look_ahead"] = {"wall": spread(rate(m["alt_wall"])), "kernel": spread(rate(m["alt_kern"]))}
    r["ratio_to_dna_decoder"] = {k: round(r["decode_msymbols_s"][k]["median"] / res["dna_decode_mbases_s"][k]["median"], 3) for k in ("wall", "kernel")}
    r["gate_at_least_dna_rate"] = all(v >= 1.0 for v in r["ratio_to_dna_decoder"].values())
    gate = gate and r["gate_at_least_dna_rate"]
    res["modes"][qm] = r
res["gate_met"] = gate
res["reference_fqs_d_t64_wall_s"] = None   # not measured here
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
