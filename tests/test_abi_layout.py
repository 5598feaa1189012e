"""The ctypes mirrors in _lib.py lay out every C-ABI struct exactly as include/diffattn.h
does: gcc compiles a probe that prints sizeof / offsetof of each field, and each ctypes
Structure must agree field by field (an appended ABI field, e.g. ABI 5's rope_freqs /
q_rot, that one side misses would shift everything after it).  CPU only."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from differential_transformer_replication_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "dta_tensor": _lib.DtaTensor,
    "dta_attn_fwd_args": _lib.AttnFwdArgs,
    "dta_attn_bwd_args": _lib.AttnBwdArgs,
    "dta_ln_args": _lib.LnArgs,
    "dta_rope_args": _lib.RopeArgs,
    "dta_attn_decode_args": _lib.DecodeArgs,
    "dta_swiglu_args": _lib.SwigluArgs,
}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_ctypes_structs_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    bad = []
    for cname, py in STRUCTS.items():
        if got[(cname, "sizeof")] != ctypes.sizeof(py):
            bad.append((cname, "sizeof", got[(cname, "sizeof")], ctypes.sizeof(py)))
        for f in py._fields_:
            off = getattr(py, f[0]).offset
            if got[(cname, f[0])] != off:
                bad.append((cname, f[0], got[(cname, f[0])], off))
    assert not bad, bad


def test_tensor5_takes_any_strides_but_a_strided_innermost_dimension():
    """dta_tensor has sb, st, sh, si and no stride for d / e: ``tensor5`` passes a view's outer
    strides through as they are and raises where the innermost dimension is not contiguous."""
    import torch
    x = torch.zeros(2, 3, 4, 2, 16)
    hm = x.permute(0, 2, 1, 3, 4)                        # head-major storage seen as [b][t][h][i][d]
    t = _lib.tensor5(hm)
    assert (t.ptr, t.sb, t.st, t.sh, t.si) == (x.data_ptr(), *hm.stride()[:4])
    v = _lib.tensor5(x[:, :, :, 1])                      # [b][t][h][e]: si unused
    assert (v.ptr, v.sb, v.st, v.sh, v.si) == (x[:, :, :, 1].data_ptr(), 384, 128, 32, 0)
    b = _lib.tensor5(x[:1].expand(2, 3, 4, 2, 16))       # a broadcast batch row: sb = 0
    assert b.sb == 0
    with pytest.raises(RuntimeError, match="innermost"):
        _lib.tensor5(x[..., ::2])
    with pytest.raises(RuntimeError, match="innermost"):
        _lib.tensor5(x.transpose(-1, -2))
    with pytest.raises(ValueError):
        _lib.tensor5(x[0, 0])
