"""FASTQ ingestion, measured: GB/s of text through
  (a) codec.parse_fastq -- upload, the parser kernels, download of the columns -- and per kernel from HIP events,
  (b) the host path it replaces: hostpipe.read_fastq, then block_arrays, id_arrays and qual_arrays over all reads, then record_sizes,
on a rectangular text (every read --len bases) and a ragged one (read lengths 2/3 --len .. --len), ids from synth.read_id.
--compress PAIRS: also compress_fastq (-p -om s -qm o -im o) on the ragged text of PAIRS pairs against compress_records_pe on
Records lists of the same reads, in Mbases/s.
A warm-up run, then --repeats timed runs; reported: median, min and max.  One JSON document on stdout (and --out).
Usage: python tools/fastq_parse_bench.py [--reads 1000000] [--len 150] [--repeats 5] [--compress 1000000] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fqsqueezer_amd import hostpipe as hp  # noqa: E402
from fqsqueezer_amd.codec import parse_fastq  # noqa: E402
from fqsqueezer_amd.synth import read_id, synth_pairs, synth_quals, synth_reads  # noqa: E402


def build_text(reads: np.ndarray, quals: np.ndarray, ragged: bool, seed: int, mate: int = 1) -> bytes:
    n, L = reads.shape
    ln = np.random.default_rng(seed).integers(2 * L // 3, L + 1, size=n) if ragged else np.full(n, L)
    return b"".join(read_id(i, mate) + b"\n" + reads[i, :ln[i]].tobytes() + b"\n+\n" + quals[i, :ln[i]].tobytes() + b"\n" for i in range(n))


def timed(fn, repeats: int):
    fn()   # warm-up
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t), "runs": repeats}


def host_path(path: str):
    rec = hp.read_fastq(path)
    idx = np.arange(len(rec), dtype=np.int64)
    return hp.block_arrays(rec, idx), hp.id_arrays(rec, idx), hp.qual_arrays(rec, idx), rec.record_sizes()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--compress", type=int, default=0, metavar="PAIRS")
    ap.add_argument("--threads", type=int, default=64)
    ap.add_argument("--gs", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"reads": a.reads, "len": a.len, "texts": {}}
    reads, quals = synth_reads(a.reads, a.len, 7_500_000, 2), synth_quals(a.reads, a.len, 2)
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("rectangular", "ragged"):
            text = build_text(reads, quals, name == "ragged", 3)
            path = os.path.join(tmp, name + ".fq")
            open(path, "wb").write(text)
            gb = len(text) / 1e9
            r = {"text_bytes": len(text)}
            st = {}
            r["parse_fastq"] = timed(lambda: parse_fastq(text, device=a.device, stats=st), a.repeats)
            r["parse_fastq_from_path"] = timed(lambda: parse_fastq(path, device=a.device), a.repeats)
            r["host_path"] = timed(lambda: host_path(path), max(2, a.repeats // 2))
            for k in ("parse_fastq", "parse_fastq_from_path", "host_path"):
                r[k]["GB_per_s"] = round(gb / r[k]["median_s"], 3)
            r["ratio_parse_over_host"] = round(r["host_path"]["median_s"] / r["parse_fastq"]["median_s"], 2)
            prof = {}
            parse_fastq(text, device=a.device, stats=prof, profile=True)   # (a run of its own: events around every launch serialise it)
            cols_bytes = st["consumed"]   # every consumed byte is read by count, index and gather; the columns are written once
            r["chunks"] = st["chunks"]
            r["kernels_ms"] = {k: round(v["ms"], 3) for k, v in prof["kernels"].items()}
            r["kernels_sum_ms"] = round(sum(v["ms"] for v in prof["kernels"].values()), 3)
            r["text_bytes_read_per_kernel_pass"] = cols_bytes
            res["texts"][name] = r
            print(name, json.dumps(r), file=sys.stderr, flush=True)
    if a.compress:
        from fqsqueezer_amd.fqsfile import compress_fastq, compress_records_pe
        n = a.compress
        r1, r2 = synth_pairs(n, a.len, 30_000_000, 4)
        q1, q2 = synth_quals(n, a.len, 4), synth_quals(n, a.len, 5)
        t1, t2 = build_text(r1, q1, True, 6, 1), build_text(r2, q2, True, 7, 2)
        with tempfile.TemporaryDirectory() as tmp:
            p1, p2 = os.path.join(tmp, "1.fq"), os.path.join(tmp, "2.fq")
            open(p1, "wb").write(t1)
            open(p2, "wb").write(t2)
            kw = dict(threads=a.threads, order="s", genome_size_mbp=a.gs, quality_mode="lossless", id_mode="lossless", device=a.device)

            def via_fastq():
                header, blocks = compress_fastq(p1, p2, as_blocks=True, **kw)
                return sum(len(c) for c in hp.fqs_chunks(header, blocks))

            rec = [hp.read_fastq(p) for p in (p1, p2)]   # (not timed: the Records path has no file reader of its own)
            bases = sum(len(x) for r in rec for x in r.seq)

            def via_records():
                header, blocks = compress_records_pe(rec[0], rec[1], kw["threads"], "s", a.gs, device=a.device, quality_mode="lossless", id_mode="lossless", as_blocks=True)
                return sum(len(c) for c in hp.fqs_chunks(header, blocks))

            assert via_fastq() == via_records()
            c = {"pairs": n, "bases": bases, "compress_fastq": timed(via_fastq, 2), "compress_records_pe": timed(via_records, 2)}
            for k in ("compress_fastq", "compress_records_pe"):
                c[k]["Mbases_per_s"] = round(bases / 1e6 / c[k]["median_s"], 2)
            res["compress_ragged_pe"] = c
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
