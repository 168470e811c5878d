"""FASTQ text assembly, measured: GB/s of text through
  (a) codec.FastqText.block + download on columns in device memory -- per kernel from HIP events (a run of its own), and for
      the whole call from a host clock around the synchronised call, block and download apart --
  (b) the host path it replaces: fqsread.fastq_text (+ _take for the two mates of a paired block) on the same columns,
on a rectangular set (every read --len bases) and a ragged one (read lengths 2/3 --len .. --len) of --reads reads, each as a
single-end and as a paired block, ids from synth.read_id.
Then the `d` command on a file this tool compresses itself (--d-reads reads, -om o -qm o -im o): wall time with gpu_text on
and off, in alternation within the one run, and the peak resident set of each and of the whole-file path that went before
(decompress_fastq on the file's bytes) from a fresh child process per variant (VmHWM of the child beside its
resource.getrusage figure, which on Linux also covers the process that launched it).
A warm-up run, then --repeats timed runs; reported: median, min and max.  One JSON document on stdout (and --out); what could
not be run is "not measured".
Usage: python tools/fastq_text_bench.py [--reads 1000000] [--len 150] [--repeats 5] [--d-reads 200000] [--out profiles/x.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fqsqueezer_amd import fqsread  # noqa: E402
from fqsqueezer_amd import hostpipe as hp  # noqa: E402
from fqsqueezer_amd.codec import FastqText  # noqa: E402
from fqsqueezer_amd.synth import read_id, synth_quals, synth_reads  # noqa: E402

NOT_MEASURED = "not measured"


def stat(t):
    return {"median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t), "runs": len(t)}


def timed(fn, repeats: int):
    fn()   # warm-up
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return stat(t)


def alternately(fns: dict, repeats: int):
    """the functions of fns in turn, a warm-up round and then `repeats` timed rounds: what one of them meets on a shared machine
    the others meet too"""
    t = {k: [] for k in fns}
    for r in range(repeats + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            if r:
                t[k].append(time.perf_counter() - t0)
    return {k: dict(stat(v), all_s=[round(x, 4) for x in v]) for k, v in t.items()}


def columns(reads: np.ndarray, quals: np.ndarray, ragged: bool, seed: int):
    n, L = reads.shape
    ln = np.random.default_rng(seed).integers(2 * L // 3, L + 1, size=n) if ragged else np.full(n, L)
    keep = np.arange(L)[None, :] < ln[:, None]
    ids = [read_id(i) + b"\n" for i in range(n)]
    off = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.uint64)   # noqa: E731
    return (np.frombuffer(b"".join(ids), dtype=np.uint8), off([len(x) for x in ids]), np.ascontiguousarray(reads[keep]), off(ln),
            np.ascontiguousarray(quals[keep]))


def assembler(a, res):
    import torch
    reads, quals = synth_reads(a.reads, a.len, 7_500_000, 2), synth_quals(a.reads, a.len, 2)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda(a.device)   # noqa: E731
    for name in ("rectangular", "ragged"):
        ids, id_off, bases, read_off, q = columns(reads, quals, name == "ragged", 3)
        id_len = np.diff(id_off.astype(np.int64)).astype(np.uint32)
        read_len = np.diff(read_off.astype(np.int64)).astype(np.uint32)
        d = [dev(x) for x in (ids, id_len, bases, q)]
        torch.cuda.synchronize()
        for paired in (False, True):
            t = FastqText(device=a.device)
            block = lambda: t.block(read_off, d[2].data_ptr(), d[3].data_ptr(), ids=d[0].data_ptr(), id_len=d[1].data_ptr(), id_bytes=len(ids), paired=paired)   # noqa: E731
            down = lambda: [t.download(m) for m in ((0, 1) if paired else (0,))]   # noqa: E731
            n_text = sum(block())
            gb = n_text / 1e9

            def host():
                text, rec_off = fqsread.fastq_text(read_len, bases, q, ids, id_off)
                if paired:
                    return [fqsread._take(text, rec_off, np.arange(m, len(read_len), 2, dtype=np.int64)) for m in (0, 1)]
                return [text]

            got, want = down(), host()
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), "the assembler and fastq_text disagree"
            r = {"text_bytes": n_text, "block": timed(block, a.repeats), "download": timed(down, a.repeats),
                 "block_and_download": timed(lambda: (block(), down()), a.repeats), "host_fastq_text": timed(host, max(2, a.repeats // 2))}
            for k in ("block", "download", "block_and_download", "host_fastq_text"):
                r[k]["GB_per_s"] = round(gb / r[k]["median_s"], 3)
            r["ratio_host_over_block_and_download"] = round(r["host_fastq_text"]["median_s"] / r["block_and_download"]["median_s"], 2)
            t.set_profiling(True)   # (a run of its own: events around every launch serialise it)
            block()
            k = t.kernel_times()
            r["kernels_ms"] = {x: round(v["ms"], 4) for x, v in k.items()}
            r["kernels_sum_ms"] = round(sum(v["ms"] for v in k.values()), 4)
            r["scatter_GB_per_s_written"] = round(gb / (k["scatter"]["ms"] / 1e3), 1) if k["scatter"]["ms"] else NOT_MEASURED
            t.close()
            res["assembler"][name + ("_paired" if paired else "_single")] = r
            print(name, paired, json.dumps(r), file=sys.stderr, flush=True)


def d_variant(variant: str, fqs: str, out: str, device: int):
    if variant == "whole_file":   # the path before the streaming one: the file and its text held whole
        text = fqsread.decompress_fastq(open(fqs, "rb").read(), device=device)
        open(out, "wb").write(text)
    else:
        fqsread.main(["d", fqs, "-out", out, "-device", str(device)] + (["-host-text"] if variant == "host_text" else []))


def child(a) -> int:
    import resource
    t0 = time.perf_counter()
    d_variant(a.child, a.fqs, a.fq_out, a.device)
    # ru_maxrss survives exec on Linux: it starts at the high-water mark of the process that launched this one, so it is
    # reported for what it is and the peak of this process's own address space is read from VmHWM
    hwm = [ln for ln in open("/proc/self/status") if ln.startswith("VmHWM:")]
    print(json.dumps({"wall_s": round(time.perf_counter() - t0, 3), "peak_rss_MiB": round(int(hwm[0].split()[1]) / 1024, 1) if hwm else NOT_MEASURED,
                      "ru_maxrss_MiB_with_the_launcher_s": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1),
                      "text_bytes": os.path.getsize(a.fq_out)}))
    return 0


def d_command(a, res):
    from fqsqueezer_amd.fqsfile import compress_records
    n = a.d_reads
    reads, quals = synth_reads(n, a.len, 7_500_000, 4), synth_quals(n, a.len, 4)
    rec = hp.Records([read_id(i) for i in range(n)], reads, quals)
    with tempfile.TemporaryDirectory() as tmp:
        fqs, out = os.path.join(tmp, "x.fqs"), os.path.join(tmp, "x.fq")
        t0 = time.perf_counter()
        header, blocks = compress_records(rec, a.threads, "o", a.gs, device=a.device, quality_mode="lossless", id_mode="lossless", as_blocks=True)
        with open(fqs, "wb") as f:
            for c in hp.fqs_chunks(header, blocks):
                f.write(c)
        r = {"reads": n, "bases": int(n) * a.len, "fqs_bytes": os.path.getsize(fqs), "compress_s": round(time.perf_counter() - t0, 2)}
        d_variant("gpu_text", fqs, out, a.device)
        want = open(out, "rb").read()
        assert want.count(b"\n") == 4 * n
        r["text_bytes"] = len(want)
        r["wall"] = alternately({v: (lambda v=v: d_variant(v, fqs, out, a.device)) for v in ("gpu_text", "host_text")}, a.d_repeats)
        assert open(out, "rb").read() == want
        g, h = r["wall"]["gpu_text"], r["wall"]["host_text"]
        r["spread_s"] = round(max(g["max_s"] - g["min_s"], h["max_s"] - h["min_s"]), 4)
        r["gpu_text_minus_host_text_median_s"] = round(g["median_s"] - h["median_s"], 4)
        r["gpu_text_not_worse_than_the_spread"] = bool(g["median_s"] - h["median_s"] <= r["spread_s"])
        r["Mbases_per_s"] = {k: round(r["bases"] / 1e6 / v["median_s"], 2) for k, v in r["wall"].items()}
        r["child"] = {}
        for v in ("gpu_text", "host_text", "whole_file"):   # a fresh process each: the peak resident set is the variant's own
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, "--fqs", fqs, "--fq-out", out, "--device", str(a.device)],
                               capture_output=True, text=True)
            r["child"][v] = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else NOT_MEASURED
        res["d_command"] = r
        print("d", json.dumps(r), file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--d-reads", type=int, default=200_000, help="reads of the file the d command is timed on (0: skip)")
    ap.add_argument("--d-repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=64)
    ap.add_argument("--gs", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fqs", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fq-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"reads": a.reads, "len": a.len, "assembler": {}, "d_command": NOT_MEASURED}
    if a.reads:
        assembler(a, res)
    if a.d_reads:
        d_command(a, res)
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
