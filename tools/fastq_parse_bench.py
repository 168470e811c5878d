"""FASTQ ingestion, measured: GB/s of text through
  (a) codec.parse_fastq -- upload, the parser kernels, download of the columns -- and per kernel from HIP events,
  (b) the host path it replaces: hostpipe.read_fastq, then block_arrays, id_arrays and qual_arrays over all reads, then record_sizes,
on a rectangular text (every read --len bases) and a ragged one (read lengths 2/3 --len .. --len), ids from synth.read_id.
--compress PAIRS: also compress_fastq (-p -om s -qm o -im o) on the ragged text of PAIRS pairs against compress_records_pe on
Records lists of the same reads, in Mbases/s, and against compress_fastq(resident=True): columns kept in device memory, blocks
cut there.  --shapes: the same for other inputs and orders (se_o, se_s: mate 1 alone; pe_o, pe_s); per shape the host-column
and the resident run alternate, and one more resident run with events around the gather launches gives the kernel's own time.
A warm-up run, then --repeats timed runs; reported: median, min and max.  One JSON document on stdout (and --out).
Usage: python tools/fastq_parse_bench.py [--reads 1000000] [--len 150] [--repeats 5] [--compress 1000000] [--shapes se_o,se_s,pe_o,pe_s]
       [--out profiles/x.json]"""
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
    return {k: {"median_s": float(np.median(v)), "min_s": min(v), "max_s": max(v), "runs": repeats} for k, v in t.items()}


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
    ap.add_argument("--shapes", default="pe_s", help="comma-separated: se_o, se_s, pe_o, pe_s")
    ap.add_argument("--compress-repeats", type=int, default=2)
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
            kw = dict(threads=a.threads, genome_size_mbp=a.gs, quality_mode="lossless", id_mode="lossless", device=a.device)
            # (a record is its id, 2 L bases and qualities, a `+` and four line feeds)
            n_bases = [(len(t) - 5 * n - sum(len(read_id(i, m + 1)) for i in range(n))) // 2 for m, t in enumerate((t1, t2))]
            for shape in a.shapes.split(","):
                ends, order = shape.split("_")
                paths = (p1, p2) if ends == "pe" else (p1,)
                bases = sum(n_bases[:len(paths)])

                def via_fastq(resident=False, stats=None, profile=False):
                    header, blocks = compress_fastq(*paths, as_blocks=True, order=order, resident=resident, stats=stats, profile=profile, **kw)
                    return sum(len(c) for c in hp.fqs_chunks(header, blocks))

                fns = {"compress_fastq": via_fastq, "compress_fastq_resident": lambda: via_fastq(True)}
                if shape == "pe_s":
                    rec = [hp.read_fastq(p) for p in (p1, p2)]   # (not timed: the Records path has no file reader of its own)
                    assert bases == sum(len(x) for r in rec for x in r.seq)

                    def via_records():
                        header, blocks = compress_records_pe(rec[0], rec[1], kw["threads"], "s", a.gs, device=a.device, quality_mode="lossless", id_mode="lossless", as_blocks=True)
                        return sum(len(c) for c in hp.fqs_chunks(header, blocks))

                    fns["compress_records_pe"] = via_records
                    assert via_fastq() == via_records()
                assert via_fastq() == via_fastq(True)
                c = dict({"pairs" if ends == "pe" else "reads": n, "bases": bases}, **alternately(fns, a.compress_repeats))
                for k in fns:
                    c[k]["Mbases_per_s"] = round(bases / 1e6 / c[k]["median_s"], 2)
                c["ratio_resident_over_host_columns"] = round(c["compress_fastq"]["median_s"] / c["compress_fastq_resident"]["median_s"], 3)
                st = {}
                via_fastq(True, st, True)   # (a run of its own: events around every gather launch)
                k = st["columns"][0]["kernels"]
                c["blocks"] = k["gather_launches"]
                c["gather_kernel_ms_per_block"] = round(k["gather_ms"] / max(1, k["gather_launches"]), 4)
                c["gather_check_ms_per_block"] = round(k["check_ms"] / max(1, k["check_launches"]), 4)
                c["columns"] = [{x: y for x, y in d.items() if x != "kernels"} for d in st["columns"]]
                res["compress_ragged_" + ("pe" if shape == "pe_s" else shape)] = c
                print(shape, json.dumps(c), file=sys.stderr, flush=True)
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
