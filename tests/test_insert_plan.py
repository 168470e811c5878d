"""The window algorithm of the insert phase (fqsx_dev.h: insert_windows) as a CPU model against the one-key-at-a-time
insert with std::mt19937(5481): tests/insert_plan_model.cpp includes the kernel's own draw rule (csrc/fqsx_insplan.h),
replays rank / decide / scan / claim / rank-round commit on a plain array table and compares counters, generator state
and the number of draws after every window.  Heavy duplication (alphabets of 1 to 200 keys, 5 000 keys a case), windows
of 1, 7, 64 and 2 048 keys, the thresholds of both counter kinds and a tiny pair (thr 1, maxv 4) that saturates inside
a window.  Built with -fsanitize=address,undefined as a program of its own and run directly."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_plan_equals_in_order_insert(tmp_path):
    exe = str(tmp_path / "insert_plan_model")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "fqsqueezer_amd", "csrc"), os.path.join(ROOT, "tests", "insert_plan_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    m = re.search(r"windows_parallel (\d+) windows_in_order (\d+) \(ambiguous (\d+)\) draws (\d+)", r.stdout)
    assert m, r.stdout
    par, in_order, ambiguous, draws = (int(x) for x in m.groups())
    assert par > 0 and in_order > 0 and ambiguous > 0 and draws > 0
