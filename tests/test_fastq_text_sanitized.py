"""The text assembler's C ABI under AddressSanitizer and UndefinedBehaviorSanitizer: tests/emu/fqtext_driver.cpp, a stand-alone
host program linked with the emulation sources (the sanitizers' runtimes are linked in; nothing is preloaded)."""
import os
import subprocess

from conftest import ROOT


def _driver():
    import __graft_entry__ as g
    bdir = os.path.join(ROOT, "build")
    os.makedirs(bdir, exist_ok=True)
    src = [os.path.join(ROOT, "tests", "emu", "fqtext_driver.cpp"), os.path.join(g.CSRC, "fqsx_api.hip"), os.path.join(g.CSRC, "fqsx_host.cpp")]
    base = ["g++", "-O1", "-g", "-std=c++17", "-DFQSX_EMU", "-ffp-contract=off", "-Wno-unused-function", "-pthread", "-x", "c++"] + src
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", os.path.join(bdir, "asan_ubsan_probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    sanitized = probe.returncode == 0
    exe = os.path.join(bdir, "fqtext_driver_san" if sanitized else "fqtext_driver")
    if not g._newer(exe, *(g._sources() + src[:1])):
        subprocess.check_call(base + (flags + ["-fno-omit-frame-pointer"] if sanitized else []) + ["-o", exe])
    return exe, sanitized


def test_assembler_cases_under_the_sanitizers(built, record_property):
    exe, sanitized = _driver()
    record_property("sanitizers", sanitized)
    print("text assembler driver:", exe, "(address + undefined sanitizers)" if sanitized else "(the compiler has no sanitizers: plain build)")
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, f"sanitized={sanitized}\n" + r.stdout[-2000:] + r.stderr[-6000:]
    n_cases, n_records = (int(x) for x in r.stdout.split("DONE")[1].split()[:2])
    assert n_cases == 36 and n_records > 20000
