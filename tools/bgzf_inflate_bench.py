"""gzip-compressed FASTQ input, measured: codec.parse_fastq end to end on one file three ways --
  (a) the plain text,
  (b) the text as BGZF (zlib level --level, --member bytes of text per member, bgzip's empty member at the end) inflated on the
      GPU (inflate="device"): compressed bytes up, one wavefront per member, the text never on the host,
  (c) the same BGZF file through zlib on the host (inflate="host"), then parsed like text --
and the inflate kernel alone from HIP events (a run of its own: events around every launch serialise it).  The text is the
benchmark's shape: --reads reads of --len bases, ids from synth.read_id.  The BGZF file is written here with Python's zlib.
A warm-up round, then --repeats rounds in which the three alternate; reported: median, min and max.  What inflate="auto" does
with BGZF (codec.BGZF_AUTO) follows from (b) against (c).  One JSON document on stdout (and --out).
Usage: python tools/bgzf_inflate_bench.py [--reads 1000000] [--len 150] [--repeats 3] [--out profiles/bgzf_inflate.json]"""
import argparse
import json
import os
import struct
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fastq_parse_bench import alternately, build_text  # noqa: E402
from fqsqueezer_amd.codec import BGZF_AUTO, parse_fastq  # noqa: E402
from fqsqueezer_amd.synth import synth_quals, synth_reads  # noqa: E402

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(text: bytes, member_bytes: int, level: int) -> bytes:
    out = []
    for i in range(0, len(text), member_bytes):
        part = text[i:i + member_bytes]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        data = c.compress(part) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(data) + 25) + data +
                   struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out) + EOF_MEMBER


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--member", type=int, default=65280)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--lib", default=None, help="path of the library to load (default: the package's libfqsx.so)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = build_text(synth_reads(a.reads, a.len, 7_500_000, 2), synth_quals(a.reads, a.len, 2), False, 3)
    gz = bgzf(text, a.member, a.level)
    res = {"reads": a.reads, "len": a.len, "level": a.level, "member_text_bytes": a.member, "text_bytes": len(text), "bgzf_bytes": len(gz),
           "members": -(-len(text) // a.member) + 1}
    with tempfile.TemporaryDirectory() as tmp:
        p_text, p_gz = os.path.join(tmp, "reads.fq"), os.path.join(tmp, "reads.fq.gz")
        open(p_text, "wb").write(text)
        open(p_gz, "wb").write(gz)
        del text, gz
        n = {}

        def run(key, path, **kw):
            st = {}
            n[key] = (len(parse_fastq(path, device=a.device, lib_path=a.lib, stats=st, **kw)), st["consumed"], st["inflate"]["where"])

        res["parse_fastq"] = alternately({"text": lambda: run("text", p_text), "bgzf_device": lambda: run("bgzf_device", p_gz, inflate="device"),
                                          "bgzf_host": lambda: run("bgzf_host", p_gz, inflate="host")}, max(3, a.repeats))
        assert n["text"][:2] == n["bgzf_device"][:2] == n["bgzf_host"][:2] and n["bgzf_device"][2] == "device" and n["bgzf_host"][2] == "host", n
        for k, r in res["parse_fastq"].items():
            r["text_GB_per_s"] = round(res["text_bytes"] / 1e9 / r["median_s"], 3)
        res["ratio_host_over_device"] = round(res["parse_fastq"]["bgzf_host"]["median_s"] / res["parse_fastq"]["bgzf_device"]["median_s"], 2)
        st = {}
        parse_fastq(p_gz, device=a.device, lib_path=a.lib, stats=st, inflate="device", profile=True)
        k = st["inflate"]
        res["inflate_kernel"] = {"ms": round(k["ms"], 3), "launches": k["launches"], "members": k["members"],
                                 "text_GB_per_s": round(res["text_bytes"] / 1e6 / k["ms"], 2) if k["ms"] else None}
        res["parser_kernels_sum_ms"] = round(sum(v["ms"] for v in st["kernels"].values()), 3)
    res["auto_should_be"] = "device" if res["ratio_host_over_device"] >= 1 else "host"
    res["auto_is"] = BGZF_AUTO
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(out + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
