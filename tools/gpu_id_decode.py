"""Rate of the id decoder (k_id_decode) against the DNA decoder on reads of the same count, in one run.
Input: n ids of synth_ids_varied and n ids of read_id, T = 64, lossless and instrument mode, in the blocks the DNA decoder
sees (n x 150 bp, se_sorted).  Every id block is encoded once (host coder), then all blocks are decoded through a fresh
decoder per pass: a warm-up pass, then `reps` passes alternating with the yardstick, the DNA decoder (fqsx_dna_decode_block).
Kernel time: HIP events (fqsx_idg_kernel_times / fqsx_dna_kernel_times); wall clock: around the decode calls of a pass,
transfers and the decoder's snapshots included.  The host twin (fqsx_id_decode_block) on one thread (T = 1) is the CPU
reference point.  No gate: the figures and the ratio ids/s : reads/s are recorded.  Writes profiles/id_decode.json.
usage: python tools/gpu_id_decode.py [--reads 1000000] [--reps 3] [--out file]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DnaCodec, IdCodec
from fqsqueezer_amd.synth import read_id, synth_ids_varied, synth_quals, synth_reads

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "id_decode.json"))
a = ap.parse_args()
n, L, T = a.reads, 150, 64
genome = max(1000000, n * L // 20)
reads = synth_reads(n, L, genome, 2)
rec = hp.Records([read_id(i) for i in range(n)], reads, synth_quals(n, L, 2))
blks = hp.form_blocks(rec, "se_sorted")


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
    t0 = time.perf_counter()
    outs = [dec.decode_block(dna_streams[g], o, g) for g, (b, o) in enumerate(dna_blocks)]
    wall = time.perf_counter() - t0
    kt = dec.kernel_times()
    dec.close()
    for out, (b, o) in zip(outs, dna_blocks):
        assert np.array_equal(out, np.asarray(b)), "DNA round trip failed"
    return wall, (kt["encode_ms"] + kt["insert_ms"] + kt["other_ms"]) / 1e3


id_sets = {"synth_ids_varied": synth_ids_varied(n, 2), "read_id": rec.ids}
cases = {}
for name, ids in id_sets.items():
    r = hp.Records(ids, reads, rec.qual)
    arrs = [hp.id_arrays(r, idx) for idx in blks]
    for im in ("lossless", "instrument"):
        c = {"header": hp.make_header(T, "se_sorted", 5, "none", im), "n": [len(off) - 1 for _, off in arrs], "wall": [], "kern": []}
        e = IdCodec(c["header"])
        c["streams"] = [e.encode_block(x, off) for x, off in arrs]
        e.close()
        h = IdCodec(c["header"])   # what has to come back: the host twin's output (the tests pin both to the reference's)
        t0 = time.perf_counter()
        c["want"] = [h.decode_block(st, k) for st, k in zip(c["streams"], c["n"])]
        c["host_T64_threads_s"] = time.perf_counter() - t0
        h.close()
        # the host twin on one thread: the same ids as one worker's
        h1 = hp.make_header(1, "se_sorted", 5, "none", im)
        e = IdCodec(h1)
        st1 = [e.encode_block(x, off) for x, off in arrs]
        e.close()
        h = IdCodec(h1)
        t0 = time.perf_counter()
        for st, k in zip(st1, c["n"]):
            h.decode_block(st, k)
        c["host_1_thread_s"] = time.perf_counter() - t0
        h.close()
        c["id_bytes"] = int(sum(int(off[-1]) for _, off in arrs))
        c["stream_bytes"] = int(sum(len(s) for st in c["streams"] for s in st))
        cases[f"{name}/{im}"] = c


def id_pass(c):
    dec = IdCodec(c["header"], device=0)
    dec.set_profiling(True)
    t0 = time.perf_counter()
    outs = [dec.decode_block(st, k) for st, k in zip(c["streams"], c["n"])]
    wall = time.perf_counter() - t0
    ms, stats = dec.kernel_times()["ms"], dec.stats()
    dec.close()
    for (ids, off), (w_ids, w_off) in zip(outs, c["want"]):
        assert np.array_equal(off, w_off) and np.array_equal(ids, w_ids), "the GPU id decoder differs from the host twin"
    return wall, ms / 1e3, stats


res = {"device": "MI355X (gfx950)", "ids": n, "read_len_of_the_yardstick": L, "T": T, "blocks": len(blks), "reps": a.reps, "cases": {}}
dna_pass(False)
for c in cases.values():
    id_pass(c)
dna_wall, dna_kern = [], []
for rep in range(a.reps):
    dna_wall.append(dna_pass(False)[0])
    for c in cases.values():
        w, k, c["stats"] = id_pass(c)
        c["wall"].append(w); c["kern"].append(k)
    dna_kern.append(dna_pass(True)[1])

res["dna_decode_kreads_s"] = {"wall": spread([n / s / 1e3 for s in dna_wall]), "kernel": spread([n / s / 1e3 for s in dna_kern])}
res["dna_decode_mbases_s"] = {k: round(v["median"] * L / 1e3, 3) for k, v in res["dna_decode_kreads_s"].items()}
for name, c in cases.items():
    r = {"decode_kids_s": {"wall": spread([n / s / 1e3 for s in c["wall"]]), "kernel": spread([n / s / 1e3 for s in c["kern"]])},
         "host_twin_1_thread_kids_s": round(n / c["host_1_thread_s"] / 1e3, 3), "host_twin_T64_threads_kids_s": round(n / c["host_T64_threads_s"] / 1e3, 3),
         "id_bytes": c["id_bytes"], "stream_bytes": c["stream_bytes"], "decoder_growth_last_pass": c["stats"]}
    r["ratio_to_dna_decoder"] = {k: round(r["decode_kids_s"][k]["median"] / res["dna_decode_kreads_s"][k]["median"], 3) for k in ("wall", "kernel")}
    r["slower_than_dna_decoder"] = any(v < 1.0 for v in r["ratio_to_dna_decoder"].values())
    res["cases"][name] = r
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(res, open(a.out, "w"), indent=1)
print(json.dumps(res))
