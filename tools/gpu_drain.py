"""Diagnostic (timing build): how long an encode launch of a small phase goes on after the last wave that the
partition / insert kernels and the next phase depend on has ended.  Runs the bench workload's first blocks through
tools/libfqsx_timing.so, reads the per-launch role time stamps (fqsx_dna_trace) and, for every launch of blocks 0-98
with seg < S, subtracts the latest end among all workers' resolving, inserter, read-head and scout waves from the latest
range-coder end: what taking the models and the coder out of the launch could remove.
usage: python tools/gpu_drain.py OUT.json [n_blocks=100] [T=64]"""
import ctypes as C, os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fqsqueezer_amd import hostpipe as hp
from fqsqueezer_amd.codec import DnaCodec
from fqsqueezer_amd.synth import synth_reads, read_id

out_path = sys.argv[1]
nblk = int(sys.argv[2]) if len(sys.argv) > 2 else 100
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
reads = synth_reads(1000000, 150, 7500000, 2)
rec = hp.Records([read_id(i) for i in range(len(reads))], reads, reads)
header = hp.make_header(T, "se_sorted", 8)
blocks = hp.form_blocks(rec, "se_sorted")[:nblk]
c = DnaCodec(header, lib_path=os.path.join(ROOT, "tools", "libfqsx_timing.so"))
where = []   # per encode launch: (block, seg, S), or None where a block's launches do not follow its schedule (growth)
irregular = 0
for g, idx in enumerate(blocks):
    bases, off = hp.block_arrays(rec, idx)
    n0 = c.kernel_times()["encode_launches"]
    c.encode_block(bases, off, g)
    n1 = c.kernel_times()["encode_launches"]
    S = max(min(100 - g if g < 100 else 0, (len(off) - 1) // T // 2) - 1, 0)   # block_prepare's schedule
    if n1 - n0 == S + 1:
        where += [(g, s, S) for s in range(S + 1)]
    else:
        where += [None] * (n1 - n0)
        irregular += 1
c._lib.fqsx_dna_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
c._lib.fqsx_dna_trace.restype = C.c_int
buf = np.zeros((4096, T, 32), dtype=np.uint64)
n = c._lib.fqsx_dna_trace(c._h, buf.ctypes.data, 4096)
tr = buf[:n].astype(np.int64)
US = 0.01   # the stamps count a 100 MHz clock

NEEDED = [1, 2, 4, 5]   # read head, resolving wave, scout, inserter: what the kernels behind the launch wait for
rows = []
for k in range(min(n, len(where))):
    if where[k] is None:
        continue
    g, seg, S = where[k]
    if g > 98 or seg >= S:
        continue
    t = tr[k]
    if not t[:, 7].any() or not t[:, 2].any():
        continue   # (a skipped launch)
    start = t[:, 0][t[:, 0] > 0].min()
    needed_end = t[:, NEEDED].max()
    rc_end = t[:, 7].max()
    models_end = t[:, 3].max()
    w = int(t[:, 7].argmax())   # the worker whose coder ends the launch
    rows.append((g, seg, (rc_end - needed_end) * US, (rc_end - start) * US, (models_end - needed_end) * US,
                 (t[w, 7] - t[w, 2]) * US, float(((t[:, 7] - t[:, 2])[t[:, 7] > 0]).mean() * US)))
a = np.array(rows, dtype=np.float64)


def dist(v):
    return {"mean": round(float(v.mean()), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2),
            **{"p%d" % q: round(float(np.percentile(v, q)), 2) for q in (5, 25, 50, 75, 95, 99)}}


def group(sel, tag):
    x = a[sel]
    if not len(x):
        return None
    d = x[:, 2]
    return {"launches": tag, "n": int(len(x)), "removable_us": dist(d), "launch_us": dist(x[:, 3]),
            "removable_share_of_launch": round(float(d.sum() / x[:, 3].sum()), 4), "removable_total_ms": round(float(np.maximum(d, 0).sum() / 1000), 2),
            "launches_where_coder_is_not_last": int((d <= 0).sum()),
            "models_end_minus_needed_end_us": dist(x[:, 4]),
            "last_coder_worker_rc_end_minus_its_resolve_end_us": dist(x[:, 5]),
            "mean_worker_rc_end_minus_resolve_end_us": dist(x[:, 6]),
            "histogram_us": {"edges": [-1e9, 0, 5, 10, 15, 20, 25, 30, 35, 40, 50, 1e9],
                             "counts": [int(v) for v in np.histogram(d, bins=[-1e9, 0, 5, 10, 15, 20, 25, 30, 35, 40, 50, 1e9])[0]]}}


res = {"what": "per encode launch of blocks 0-98 with seg < S: latest range-coder end minus the latest end of any worker's read-head, "
               "scout, resolving or inserter wave (timing build, role stamps 1, 2, 4, 5 against 7)",
       "workload": "bench.py's: 1 M x 150 bp single-end sorted, T = %d, first %d blocks" % (T, nblk),
       "trace_launches": int(n), "blocks_off_schedule": irregular,
       "groups": [r for r in (group(a[:, 0] >= 0, "blocks 0..98, seg < S"), group(a[:, 0] < 70, "blocks 0..69"),
                              group(a[:, 0] >= 70, "blocks 70..98")) if r]}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res["groups"][0]))
