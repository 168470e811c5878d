"""The resident id column, measured against the route it replaces on the same input (--reads x --len bp with synth's
Illumina-style ids, -t --threads, the blocks the file layer forms for original order), in one process after a warm-up:
  per block  (a) the parent's route: hostpipe.Columns.ids_of(idx) (numpy gather of the block's id lines) + IdCodec.encode_block
                 (host pass over the bytes for the table sizes, upload, kernel);
             (b) DeviceColumns.ids_dev(idx) (the lines cut on the device) + IdCodec.encode_block_dev (separators counted by a
                 kernel, the id kernel on the block where it lies).
             Both on the GPU id coder, a fresh pair of codecs per round, the two routes in turn block by block on a host clock
             around calls that end in a synchronise; the streams of the two are compared.  Per round the mean time of a block;
             reported: median, min, max and spread (max - min) over the --repeats timed rounds, and the same for the gather alone.
             The condition recorded: (b)'s median is not above (a)'s by more than (a)'s own spread.
  kernels    the id gather's two passes, the separator count and the survey, from the handles' profiling events (one more
             round with profiling on).
  whole file compress_fastq(resident=True) against compress_fastq(resident=True, resident_ids=True), -om s -qm 8 -im o, in
             turn; Mbases/s of each (no threshold).  The two files are compared.
Usage: python tools/resident_ids_bench.py [--reads 1000000] [--len 150] [--threads 64] [--repeats 3] [--out profiles/resident_ids_ab.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fqsqueezer_amd import fqsread  # noqa: E402
from fqsqueezer_amd import hostpipe as hp  # noqa: E402
from fqsqueezer_amd.codec import IdCodec, parse_fastq  # noqa: E402
from fqsqueezer_amd.fqsfile import compress_fastq  # noqa: E402
from fqsqueezer_amd.synth import synth_ids_varied, synth_quals, synth_reads  # noqa: E402

NOT_MEASURED = "not measured"


def stat(t):
    return {"median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t), "spread_s": max(t) - min(t), "all_s": [round(x, 6) for x in t]}


def write_text(path: str, n: int, L: int) -> int:
    reads, quals = synth_reads(n, L, 7_500_000, 2), synth_quals(n, L, 2)
    ids = [x + b"\n" for x in synth_ids_varied(n, 2)]
    id_off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.uint64)
    text, _ = fqsread.fastq_text(np.full(n, L, dtype=np.uint32), np.ascontiguousarray(reads).reshape(-1), np.ascontiguousarray(quals).reshape(-1),
                                 np.frombuffer(b"".join(ids), dtype=np.uint8), id_off)
    text.tofile(path)
    return len(text)


def per_block(a, res) -> None:
    host = parse_fastq(a.text, device=a.device, lib_path=a.lib, max_chunk_bytes=a.chunk_bytes)
    store = parse_fastq(a.text, device=a.device, lib_path=a.lib, max_chunk_bytes=a.chunk_bytes, resident=True, resident_ids=True)
    try:
        header = hp.make_header(a.threads, "se_original", 3100, id_mode="lossless")
        blocks = hp.form_blocks(host, "se_original")
        res["blocks"], res["reads_per_block"] = len(blocks), [len(b) for b in blocks[:3]]
        res["id_bytes"], res["store"] = len(host.ids), store.info()
        t = {"a_ids_of": [], "a_encode_block": [], "a": [], "b_ids_dev": [], "b_encode_block_dev": [], "b": []}
        for r in range(a.repeats + 1):   # round 0 warms up
            ca, cb = IdCodec(header, lib_path=a.lib, device=a.device), IdCodec(header, lib_path=a.lib, device=a.device)
            s = dict.fromkeys(t, 0.0)
            for idx in blocks:   # in turn: what one meets on a shared machine the other meets too
                t0 = time.perf_counter()
                ids, off = host.ids_of(idx)
                t1 = time.perf_counter()
                want = ca.encode_block(ids, off)
                t2 = time.perf_counter()
                blk = store.ids_dev(idx)
                t3 = time.perf_counter()
                got = cb.encode_block_dev(blk.ids, blk.d_off, blk.off)
                t4 = time.perf_counter()
                assert got == want, "the two routes disagree"
                for k, v in (("a_ids_of", t1 - t0), ("a_encode_block", t2 - t1), ("a", t2 - t0), ("b_ids_dev", t3 - t2), ("b_encode_block_dev", t4 - t3), ("b", t4 - t2)):
                    s[k] += v
            assert ca.stats() == cb.stats() and np.array_equal(ca.state(), cb.state())
            ca.close(); cb.close()
            if r:
                for k in t:
                    t[k].append(s[k] / len(blocks))
        res["per_block"] = {k: stat(v) for k, v in t.items()}
        a_, b_ = res["per_block"]["a"], res["per_block"]["b"]
        res["b_minus_a_median_s"] = round(b_["median_s"] - a_["median_s"], 6)
        res["b_not_above_a_by_more_than_its_spread"] = bool(b_["median_s"] - a_["median_s"] <= a_["spread_s"])
        # ---- kernel times: one more round, every launch between the handle's two events
        store.set_profiling(True)
        cb = IdCodec(header, lib_path=a.lib, device=a.device)
        cb.set_profiling(True)
        res["survey"] = store.id_survey()
        for idx in blocks:
            blk = store.ids_dev(idx)
            cb.encode_block_dev(blk.ids, blk.d_off, blk.off)
        ks, kc = store.kernel_times(), cb.kernel_times()
        cb.close()
        n = len(blocks)
        res["kernels_ms"] = {"id_gather_check_per_block": ks["id_check_ms"] / n, "id_gather_copy_per_block": ks["id_gather_ms"] / n,
                             "separator_count_per_block": kc["separators_ms"] / n, "id_encode_per_block": kc["ms"] / n,
                             "id_survey_whole_file": ks["id_survey_ms"],
                             "launches": {"id_check": ks["id_check_launches"], "id_gather": ks["id_gather_launches"],
                                          "separators": kc["separators_launches"], "id_encode": kc["launches"], "id_survey": ks["id_survey_launches"]}}
    finally:
        store.close()


def whole_file(a, res) -> None:
    kw = dict(threads=a.threads, order="s", quality_mode="illumina_8", id_mode="lossless", device=a.device, lib_path=a.lib, max_chunk_bytes=a.chunk_bytes, resident=True)
    t, size = {"resident": [], "resident_ids": []}, {}
    for r in range(a.file_repeats + 1):   # round 0 warms up
        for k, extra in (("resident", {}), ("resident_ids", {"resident_ids": True})):
            st = {}
            t0 = time.perf_counter()
            data = compress_fastq(a.text, stats=st, **kw, **extra)
            dt = time.perf_counter() - t0
            if r:
                t[k].append(dt)
            if k == "resident":
                want = data
            else:
                assert data == want, "the two files differ"
                assert st["ids_resident"] and st["gpu_ids"] and not st["id_host_fallback"]
            size[k] = len(data)
    mbases = a.reads * a.len / 1e6
    res["whole_file"] = {k: dict(stat(v), Mbases_per_s=round(mbases / float(np.median(v)), 2), file_bytes=size[k]) for k, v in t.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--threads", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--file-repeats", type=int, default=2, help="timed whole-file rounds (0: skip the whole-file part)")
    ap.add_argument("--chunk-bytes", type=int, default=64 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    res = {"reads": a.reads, "len": a.len, "threads": a.threads, "chunk_bytes": a.chunk_bytes, "per_block": NOT_MEASURED, "kernels_ms": NOT_MEASURED,
           "whole_file": NOT_MEASURED}
    with tempfile.TemporaryDirectory() as tmp:
        a.text = os.path.join(tmp, "x.fq")
        res["text_bytes"] = write_text(a.text, a.reads, a.len)
        per_block(a, res)
        if a.file_repeats:
            whole_file(a, res)
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
