"""The product library: builds, exports every symbol include/fqsx.h declares, and has no CPU path."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def libpath():
    import __graft_entry__ as g
    return g.build_hip()


def test_exports_every_declared_symbol(libpath):
    hdr = open(os.path.join(ROOT, "include", "fqsx.h")).read()
    declared = set(re.findall(r"\b(fqsx_[a-z_]+)\s*\(", hdr))
    assert {"fqsx_dna_create", "fqsx_dna_encode_block", "fqsx_dna_encode_block_dev", "fqsx_dna_destroy",
            "fqsx_last_error"} <= declared
    lib = C.CDLL(libpath)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/fqsx.h but not exported"


def test_codec_binds_every_function_it_calls_when_the_library_is_loaded(built):
    """codec.py has one table of signatures, applied by load_library: every fqsx_* function the module calls -- as an
    attribute of the library or by its name, given to a call helper -- is a key of it, every key is declared in
    include/fqsx.h, and a loaded library (the emulation build) has each of them bound."""
    import ast
    from conftest import EMU_LIB
    from fqsqueezer_amd import codec
    tree = ast.parse(open(os.path.join(ROOT, "fqsqueezer_amd", "codec.py")).read())
    table = next(n for n in tree.body if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "_ABI" for t in n.targets))
    in_table = {id(n) for n in ast.walk(table)}
    called = set()
    for n in ast.walk(tree):
        if id(n) in in_table:
            continue
        if isinstance(n, ast.Attribute) and n.attr.startswith("fqsx_"):
            called.add(n.attr)
        elif isinstance(n, ast.Constant) and isinstance(n.value, str) and re.fullmatch(r"fqsx_[a-z0-9_]+", n.value):
            called.add(n.value)
    assert {"fqsx_dna_encode_block", "fqsx_idg_decode_block_dev", "fqsx_fqtext_block", "fqsx_cols_gather", "fqsx_last_error"} <= called
    assert called <= set(codec._ABI), sorted(called - set(codec._ABI))
    declared = set(re.findall(r"\b(fqsx_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "fqsx.h")).read()))
    assert set(codec._ABI) <= declared, sorted(set(codec._ABI) - declared)
    lib = codec.load_library(EMU_LIB)
    for name in codec._ABI:
        assert getattr(lib, name).argtypes is not None, f"{name} is not bound by load_library"


def test_contains_gfx950_code_object(libpath):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", libpath], capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(libpath, "rb").read()
    for kernel in (b"k_encode_se_sorted", b"k_encode_se_orig", b"k_encode_pe_sorted", b"k_decode_se_sorted", b"k_insert_phase", b"k_qual_encode"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob


def test_fails_loudly_without_gpu(libpath):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fqsqueezer_amd import hostpipe as hp
    lib = C.CDLL(libpath)
    lib.fqsx_last_error.restype = C.c_char_p
    h = C.c_void_p()
    rc = lib.fqsx_dna_create(hp.make_header(2, "se_sorted", 1), 0, C.byref(h))
    assert rc == -2 and not h.value                       # FQSX_E_NO_DEVICE
    assert b"no CPU path" in lib.fqsx_last_error()


def test_package_never_selects_emulation():
    src = open(os.path.join(ROOT, "fqsqueezer_amd", "codec.py")).read()
    assert "libfqsx_emu" not in src.replace("host-emulation", "")
    for f in os.listdir(os.path.join(ROOT, "fqsqueezer_amd")):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(ROOT, "fqsqueezer_amd", f)).read().replace("# oracle", "")
