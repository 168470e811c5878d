"""bench.py on one MI355X at a small size: a plain run measures the headline and nothing else; `--full` adds the passes
beside it and leaves the headline's output unchanged."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--reads", "20000", "--genome", "200000"]
EXTRAS = ("roofline", "cpu_baseline", "pcie_inclusive_mbases_s", "workers_255", "concurrent_files", "other_rows", "large_file")


def bench_line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def test_plain_and_full_bench_runs(tmp_path):
    plain = bench_line("--dump-outputs", str(tmp_path))
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "Mbases/s" and plain["higher_is_better"] is True
    assert all(plain[k] is None for k in EXTRAS), {k: plain[k] for k in EXTRAS if plain[k] is not None}
    assert (tmp_path / "dna_stream_bytes.npy").exists() and (tmp_path / "dna_streams.npy").exists()

    full = bench_line("--full", "--no-cpu-baseline", "--no-rows", "--concurrent", "0")
    assert full["roofline"]["launches"] > 0 and full["roofline"]["kernel"] in ("k_encode_se_sorted", "k_insert_phase")
    assert full["pcie_inclusive_mbases_s"] > 0 and full["workers_255"]["value"] > 0
    assert full["bits_per_base"] == plain["bits_per_base"] and full["capacity"]["bmers"] == plain["capacity"]["bmers"]
