"""ABI 9: ``_lib.ExtendArgs`` lays out ``dta_attn_extend_args`` exactly as
include/diffattn.h does (the gcc sizeof / offsetof probe of test_abi_layout.py), and the
built library reports ABI version 9 and exports the new symbols.  CPU only."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from differential_transformer_replication_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_extend_args_match_the_header():
    cname, py = "dta_attn_extend_args", _lib.ExtendArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ['  printf("abi %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert got["abi"] == _lib.ABI_VERSION == 9
    assert got["sizeof"] == ctypes.sizeof(py)
    bad = [(f[0], got[f[0]], getattr(py, f[0]).offset) for f in py._fields_ if got[f[0]] != getattr(py, f[0]).offset]
    assert not bad, bad


def test_built_library_is_abi_9():
    lib = _lib.load()                     # the library build() left in the tree; raises on an ABI mismatch
    assert lib.dta_abi_version() == 9
    for name in ("dta_attn_extend", "dta_extend_supported"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # the support query needs no device: head sizes % 16 up to 128, dv % 32 up to 256, N <= 8
    assert lib.dta_extend_supported(_lib.DTA_BF16, 64, 2, 128) == 1
    assert lib.dta_extend_supported(_lib.DTA_F32, 128, 8, 256) == 1
    assert lib.dta_extend_supported(_lib.DTA_F32, 40, 2, 80) == 0
    assert lib.dta_extend_supported(_lib.DTA_F16, 64, 9, 128) == 0
