"""The sorted-order pre-pass of a resident store, measured two ways on the same store (--reads x --len bp, parsed in chunks of
--chunk-bytes of text):
  (a) the route before DeviceColumns.sort_order: bases_to_host() (the whole base column to the host) + codec.sort_order on it
      (binning on the host, the column uploaded again, the sort on a context of its own);
  (b) DeviceColumns.sort_order(): the store's reads located and sorted where they lie.
In alternation within the one process, a warm-up round and then --repeats timed rounds on a host clock around the synchronous
calls; reported: median, min, max, spread (max - min) and every time.  The two orders are compared.  Then a fresh child process
per variant parses the same file into a resident store and runs the variant once: the store's device_bytes_peak (the host
route's second copy of the column is on another context and is reported as what that context asks for: bases + 8 (n + 1)
bytes of offsets + 16 n of the sort's own arrays), and the child's peak resident set (VmHWM).
The condition recorded: (b)'s median is not above (a)'s by more than (a)'s own spread.
Usage: python tools/resident_sort_bench.py [--reads 1000000] [--len 150] [--repeats 3] [--out profiles/resident_sort_ab.json]"""
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
from fqsqueezer_amd.codec import parse_fastq, sort_order  # noqa: E402
from fqsqueezer_amd.synth import read_id, synth_quals, synth_reads  # noqa: E402

NOT_MEASURED = "not measured"


def stat(t):
    return {"median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t), "spread_s": max(t) - min(t), "all_s": [round(x, 4) for x in t]}


def write_text(path: str, n: int, L: int) -> int:
    reads, quals = synth_reads(n, L, 7_500_000, 2), synth_quals(n, L, 2)
    ids = [read_id(i) + b"\n" for i in range(n)]
    id_off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.uint64)
    text, _ = fqsread.fastq_text(np.full(n, L, dtype=np.uint32), np.ascontiguousarray(reads).reshape(-1), np.ascontiguousarray(quals).reshape(-1),
                                 np.frombuffer(b"".join(ids), dtype=np.uint8), id_off)
    text.tofile(path)
    return len(text)


def variants(store, device: int):
    def host_route():
        return sort_order(store.bases_to_host(), store.read_off, device=device)

    def resident_route():
        st = {}
        return store.sort_order(stats=st), st
    return host_route, resident_route


def child(a) -> int:
    t0 = time.perf_counter()
    st = {}
    store = parse_fastq(a.text, device=a.device, max_chunk_bytes=a.chunk_bytes, stats=st, resident=True)
    held = store.info()["device_bytes"]
    host_route, resident_route = variants(store, a.device)
    t1 = time.perf_counter()
    sort_stats = resident_route()[1] if a.child == "resident" else (host_route(), {})[1]
    t2 = time.perf_counter()
    info = store.info()
    store.close()
    hwm = [ln for ln in open("/proc/self/status") if ln.startswith("VmHWM:")]
    print(json.dumps({"chunks": st["chunks"], "store_device_bytes": held, "store_device_bytes_peak": info["device_bytes_peak"],
                      "store_peak_above_held": info["device_bytes_peak"] - held, "sort": sort_stats, "pre_pass_s": round(t2 - t1, 4),
                      "wall_s": round(time.perf_counter() - t0, 3), "peak_rss_MiB": round(int(hwm[0].split()[1]) / 1024, 1) if hwm else NOT_MEASURED}))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=64 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--text", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"reads": a.reads, "len": a.len, "chunk_bytes": a.chunk_bytes, "whole_file_against_the_parent_commit": NOT_MEASURED}
    with tempfile.TemporaryDirectory() as tmp:
        a.text = os.path.join(tmp, "x.fq")
        res["text_bytes"] = write_text(a.text, a.reads, a.len)
        st = {}
        store = parse_fastq(a.text, device=a.device, max_chunk_bytes=a.chunk_bytes, stats=st, resident=True)
        res["chunks"], res["store"] = st["chunks"], store.info()
        host_route, resident_route = variants(store, a.device)
        t = {"host_route": [], "resident": []}
        for r in range(a.repeats + 1):   # in turn: what one meets on a shared machine the other meets too; round 0 warms up
            for k, fn in (("host_route", host_route), ("resident", resident_route)):
                t0 = time.perf_counter()
                got = fn()
                if r:
                    t[k].append(time.perf_counter() - t0)
                if k == "host_route":
                    want = got
                else:
                    res["sort"] = got[1]
                    assert len(got[0]) == len(want) and all(np.array_equal(x, y) for x, y in zip(got[0], want)), "the two routes disagree"
        res["store_after"] = store.info()
        store.close()
        res["pre_pass"] = {k: stat(v) for k, v in t.items()}
        a_, b_ = res["pre_pass"]["host_route"], res["pre_pass"]["resident"]
        res["resident_minus_host_route_median_s"] = round(b_["median_s"] - a_["median_s"], 4)
        res["resident_not_above_host_route_by_more_than_its_spread"] = bool(b_["median_s"] - a_["median_s"] <= a_["spread_s"])
        res["host_route_second_copy_bytes"] = a.reads * a.len + 8 * (a.reads + 1) + 16 * a.reads
        res["child"] = {}
        for v in ("host_route", "resident"):   # a fresh process each: the peaks are the variant's own
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, "--text", a.text, "--device", str(a.device),
                                "--chunk-bytes", str(a.chunk_bytes)], capture_output=True, text=True)
            res["child"][v] = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else NOT_MEASURED
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
