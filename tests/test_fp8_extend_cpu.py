"""CPU checks of the multi-row step on the fp8 (e4m3fn) paged KV cache: the two entry points
(``dta_attn_extend_paged_fp8``, ``dta_extend_fp8_supported``) are in the header and in the built
library inside ABI 9, ``_lib.ExtendPagedFp8Args`` lays its struct out as include/diffattn.h does
(the gcc probe of test_fp8_cache_cpu.py), the support query answers for the shapes both the
extend plans and the quantising write take, the entry point rejects bad arguments wherever it
returns before a launch, and ``kv_cache.PagedKVCache`` takes and checks ``fp8_extend``."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_fp8_extend_args_match_the_header():
    cname, py = "dta_attn_extend_paged_fp8_args", _lib.ExtendPagedFp8Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    # sizeof of a call is not evaluated, so nothing links, and an undeclared or differently typed
    # function does not compile
    lines += [f'  printf("declared %zu\\n", sizeof(dta_attn_extend_paged_fp8((const {cname}*)0, (void*)0))'
              ' / sizeof(dta_extend_fp8_supported(0, 64, 2, 128)));',
              '  printf("abi %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-Werror=implicit-function-declaration", "-I", os.path.join(ROOT, "include"),
                        src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got["abi"] == _lib.ABI_VERSION == 9                      # the feature arrives without an ABI bump
    assert got["declared"] == 1
    assert got["sizeof"] == ctypes.sizeof(py)
    bad = [(f[0], got[f[0]], getattr(py, f[0]).offset) for f in py._fields_ if got[f[0]] != getattr(py, f[0]).offset]
    assert not bad, bad
    # the fp8 extend struct is the paged one with the scale pool appended, as the decode one is
    assert ([f[0] for f in _lib.ExtendPagedArgs._fields_] + ["scale_pool_dev", "scale_page_stride"]
            == [f[0] for f in py._fields_])


def test_exports_and_support_queries():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.FP8_EXTEND_EXPORTS == ("dta_attn_extend_paged_fp8", "dta_extend_fp8_supported")
    for name in _lib.FP8_EXTEND_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.fp8_extend_symbols(lib)

    class _Old:                                   # a library with the fp8 cache but without the extend step
        dta_attn_decode_paged_fp8 = dta_kv_quant_rows = dta_attn_extend_paged = None
    assert _lib.fp8_symbols(_Old()) and not _lib.fp8_extend_symbols(_Old())

    sup = lib.dta_extend_fp8_supported
    assert sup(_lib.DTA_BF16, 64, 2, 128) == 1
    assert sup(_lib.DTA_F32, 128, 4, 256) == 1
    assert sup(_lib.DTA_F16, 16, 1, 32) == 1
    assert sup(_lib.DTA_BF16, 40, 2, 128) == 0     # head size not a multiple of 16
    assert sup(_lib.DTA_BF16, 64, 5, 128) == 0     # the quantising write stops at 4 branches
    assert sup(_lib.DTA_BF16, 64, 2, 48) == 0      # dv not a multiple of 32
    assert sup(3, 64, 2, 128) == 0                 # no such dtype
    assert ops.extend_fp8_supported(torch.bfloat16, 64, 2, 128) is True
    assert ops.extend_fp8_supported(torch.float32, 24, 2, 48) is False


def _args(**kw):
    """An fp8 paged extend call that passes every host check at B = 0, so no pointer is
    dereferenced and nothing is launched (the scheme of test_fp8_cache_cpu._decode_args)."""
    a = _lib.ExtendPagedFp8Args()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 2, 2, 64, 128
    a.Tq, a.t_cap, a.scale = 5, 128, 0.125
    a.page_size, a.max_pages, a.n_pages = 64, 2, 4
    buf = (ctypes.c_int32 * 8)()
    a.pos_dev = ctypes.addressof(buf)
    a.block_table_dev = ctypes.addressof(buf)
    a.scale_pool_dev = ctypes.addressof(buf)
    a.scale_page_stride = 64 * 2 * 3
    a.k_pool.sb, a.k_pool.st, a.k_pool.sh, a.k_pool.si = 64 * 512, 512, 128, 64
    a.v_pool.sb, a.v_pool.st, a.v_pool.sh = 64 * 512, 512, 128
    a._keep = buf
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split("__")
        for name in path:
            obj = getattr(obj, name)
        setattr(obj, leaf, v)
    return a


def test_entry_point_rejects_bad_arguments_without_a_device():
    ext = _lib.load().dta_attn_extend_paged_fp8
    base = _args()
    assert ext(None, None) == -1
    assert ext(ctypes.byref(_lib.ExtendPagedFp8Args()), None) == -1
    assert ext(ctypes.byref(_args()), None) == 0                                      # B = 0: valid, no launch
    assert ext(ctypes.byref(_args(Tq=0, B=2)), None) == 0                             # Tq = 0 likewise
    assert ext(ctypes.byref(_args(count_dev=base.pos_dev)), None) == 0
    # everything dta_attn_extend_paged rejects
    assert ext(ctypes.byref(_args(page_size=32, max_pages=4, scale_page_stride=32 * 6)), None) == 0
    assert ext(ctypes.byref(_args(page_size=256, max_pages=1, t_cap=256, scale_page_stride=256 * 6)), None) == 0
    assert ext(ctypes.byref(_args(page_size=48, max_pages=2, t_cap=96)), None) == -1
    assert ext(ctypes.byref(_args(page_size=512, max_pages=1, t_cap=512, scale_page_stride=512 * 6)), None) == -1
    assert ext(ctypes.byref(_args(t_cap=127)), None) == -1                            # != max_pages * page_size
    assert ext(ctypes.byref(_args(max_pages=3)), None) == -1
    assert ext(ctypes.byref(_args(n_pages=0)), None) == -1
    assert ext(ctypes.byref(_args(block_table_dev=None)), None) == -1
    assert ext(ctypes.byref(_args(block_table_dev=base.block_table_dev + 2)), None) == -1
    assert ext(ctypes.byref(_args(pos_dev=None)), None) == -1
    assert ext(ctypes.byref(_args(pos_dev=base.pos_dev + 1)), None) == -1
    assert ext(ctypes.byref(_args(count_dev=base.pos_dev + 2)), None) == -1
    assert ext(ctypes.byref(_args(dtype=3)), None) == -1
    assert ext(ctypes.byref(_args(Tq=-1)), None) == -1
    assert ext(ctypes.byref(_args(Tq=128)), None) == 0
    assert ext(ctypes.byref(_args(Tq=129)), None) == -1                               # pos + Tq > t_cap
    # the fp8 arguments
    assert ext(ctypes.byref(_args(scale_pool_dev=None)), None) == -1
    assert ext(ctypes.byref(_args(scale_pool_dev=base.scale_pool_dev + 2)), None) == -1
    assert ext(ctypes.byref(_args(scale_page_stride=64 * 2 * 3 - 1)), None) == -1
    assert ext(ctypes.byref(_args(scale_page_stride=64 * 2 * 3 + 5)), None) == 0      # padding between pages is fine
    for field in ("k_pool__sb", "k_pool__st", "v_pool__sb", "v_pool__st"):
        assert ext(ctypes.byref(_args(**{field: 520})), None) == -1, field            # 520 % 16 == 8
        assert ext(ctypes.byref(_args(**{field: 528})), None) == 0, field
    # shapes without a plan: where dta_extend_fp8_supported is 0
    for bad in (dict(head_size=40), dict(head_size=144), dict(dv=48), dict(dv=288),
                dict(n_terms=5, scale_page_stride=64 * 2 * 6)):
        assert ext(ctypes.byref(_args(**bad)), None) == -2, bad
    # with rows to run, the operands are checked before any launch: null tensors
    assert ext(ctypes.byref(_args(B=1)), None) == -1


def test_cache_constructor_takes_fp8_extend():
    with pytest.raises(ValueError):
        kv_cache.PagedKVCache(4, 32, fp8_extend=True)
    with pytest.raises(ValueError):
        kv_cache.PagedKVCache(4, 32, kv_dtype=None, fp8_extend=True)
    on = kv_cache.PagedKVCache(4, 32, kv_dtype="fp8_e4m3", fp8_extend=True)
    off = kv_cache.PagedKVCache(4, 32, kv_dtype="fp8_e4m3")
    assert on.fp8_extend is True and on.kv_dtype == "fp8_e4m3"
    assert off.fp8_extend is False
    assert kv_cache.PagedKVCache(4, 32).fp8_extend is False
