"""Host side of the multi-row split-key decode (no GPU): the ctypes structs against the
header, the export list, the argument checks of the three entry points (at B = 0, so no
pointer is dereferenced and nothing is launched), and the dispatch of ``rows_decode``."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "dta_attn_decode_rows_args": _lib.DecodeRowsArgs,
    "dta_attn_decode_rows_paged_args": _lib.DecodeRowsPagedArgs,
    "dta_attn_decode_rows_paged_fp8_args": _lib.DecodeRowsPagedFp8Args,
}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_rows_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    # sizeof of a call is not evaluated: nothing links, and an undeclared or differently typed
    # function does not compile
    lines += ['  printf("symbols declared %zu\\n", sizeof(dta_attn_decode_rows((const dta_attn_decode_rows_args*)0, (void*)0))'
              ' / sizeof(dta_attn_decode_rows_paged((const dta_attn_decode_rows_paged_args*)0, (void*)0))'
              ' * sizeof(dta_attn_decode_rows_paged_fp8((const dta_attn_decode_rows_paged_fp8_args*)0, (void*)0))'
              ' / sizeof(dta_decode_rows_supported(0, 0, 0, 0, 0, 0))'
              ' * sizeof(dta_attn_decode_rows_workspace_bytes(0, 0, 0, 0, 0, 0, 0)) / sizeof(size_t));',
              '  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-Werror=implicit-function-declaration", "-I", os.path.join(ROOT, "include"),
                        src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    assert got[("abi", "version")] == _lib.ABI_VERSION == 9         # the feature arrives without an ABI bump
    assert got[("symbols", "declared")] == 1
    bad = []
    for cname, py in STRUCTS.items():
        if got[(cname, "sizeof")] != ctypes.sizeof(py):
            bad.append((cname, "sizeof", got[(cname, "sizeof")], ctypes.sizeof(py)))
        for f in py._fields_:
            off = getattr(py, f[0]).offset
            if got[(cname, f[0])] != off:
                bad.append((cname, f[0], got[(cname, f[0])], off))
    assert not bad, bad
    # the paged struct is the contiguous one with the pool views and the table appended, the fp8 one
    # the paged one with the scale pool appended
    names = lambda py: [f[0] for f in py._fields_]
    assert ([n.replace("_cache", "_pool") for n in names(_lib.DecodeRowsArgs)]
            + ["page_size", "max_pages", "n_pages", "block_table_dev"] == names(_lib.DecodeRowsPagedArgs))
    assert names(_lib.DecodeRowsPagedArgs) + ["scale_pool_dev", "scale_page_stride"] == names(_lib.DecodeRowsPagedFp8Args)


def test_rows_exports():
    assert _lib.ROWS_EXPORTS == ("dta_attn_decode_rows", "dta_attn_decode_rows_paged", "dta_attn_decode_rows_paged_fp8",
                                 "dta_attn_decode_rows_workspace_bytes", "dta_decode_rows_supported")
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    for name in _lib.ROWS_EXPORTS:
        assert hasattr(lib, name), name
    assert _lib.rows_symbols(lib)

    class _Old:                                   # a library of the same ABI without the symbols
        dta_attn_decode_paged_fp8 = dta_attn_extend_paged_fp8 = None
    assert not _lib.rows_symbols(_Old())


def _args(cls=_lib.DecodeRowsPagedFp8Args, **kw):
    """A call that passes every host check at B = 0 (the scheme of test_fp8_cache_cpu._decode_args)."""
    a = cls()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 2, 2, 64, 128
    a.Tq, a.t_cap, a.scale = 4, 128, 0.125
    buf = (ctypes.c_int32 * 8)()
    a.pos_dev = ctypes.addressof(buf)
    a._keep = buf
    if cls is not _lib.DecodeRowsArgs:
        a.page_size, a.max_pages, a.n_pages = 64, 2, 4
        a.block_table_dev = ctypes.addressof(buf)
        a.k_pool.sb, a.k_pool.st, a.k_pool.sh, a.k_pool.si = 64 * 512, 512, 128, 64
        a.v_pool.sb, a.v_pool.st, a.v_pool.sh = 64 * 512, 512, 128
    if cls is _lib.DecodeRowsPagedFp8Args:
        a.scale_pool_dev = ctypes.addressof(buf)
        a.scale_page_stride = 64 * 2 * 3
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split("__")
        for name in path:
            obj = getattr(obj, name)
        setattr(obj, leaf, v)
    return a


def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    entries = ((lib.dta_attn_decode_rows, _lib.DecodeRowsArgs), (lib.dta_attn_decode_rows_paged, _lib.DecodeRowsPagedArgs),
               (lib.dta_attn_decode_rows_paged_fp8, _lib.DecodeRowsPagedFp8Args))
    for fn, cls in entries:
        call = lambda **kw: fn(ctypes.byref(_args(cls, **kw)), None)
        assert fn(None, None) == -1
        assert fn(ctypes.byref(cls()), None) == -1
        assert call() == 0                                           # B = 0: valid, no launch
        assert call(Tq=1) == 0 and call(Tq=8) == 0
        assert call(Tq=0) == -1 and call(Tq=9) == -1 and call(Tq=-1) == -1
        assert call(pos_dev=None) == -1
        assert call(pos_dev=_args(cls).pos_dev + 2) == -1            # not 4-byte aligned
        assert call(count_dev=_args(cls).pos_dev + 1) == -1
        assert call(count_dev=_args(cls).pos_dev + 4) == 0
        assert call(dtype=3) == -1 and call(B=-1) == -1 and call(H=0) == -1
        assert call(t_cap=3) == -1                                   # t_cap < Tq
        for bad in (dict(head_size=40, dv=80), dict(head_size=16, dv=32), dict(n_terms=5), dict(dv=64), dict(head_size=132)):
            if "n_terms" in bad and cls is _lib.DecodeRowsPagedFp8Args:
                bad["scale_page_stride"] = 64 * 2 * 6
            assert call(**bad) == -2, bad                            # no split plan: unsupported, no other kernel
        assert call(n_terms=1, dv=64) == 0
    for fn, cls in entries[1:]:
        call = lambda **kw: fn(ctypes.byref(_args(cls, **kw)), None)
        assert call(block_table_dev=None) == -1
        assert call(block_table_dev=_args(cls).block_table_dev + 2) == -1                 # misaligned table
        assert call(t_cap=127) == -1 and call(max_pages=3) == -1                          # t_cap != max_pages * page_size
        assert call(page_size=48, max_pages=2, t_cap=96) == -1
        assert call(n_pages=0) == -1
    call = lambda **kw: entries[2][0](ctypes.byref(_args(**kw)), None)
    assert call(page_size=32, max_pages=4, scale_page_stride=32 * 6) == 0
    assert call(scale_pool_dev=None) == -1
    assert call(scale_pool_dev=_args().scale_pool_dev + 2) == -1
    assert call(scale_page_stride=64 * 2 * 3 - 1) == -1
    for field in ("k_pool__sb", "k_pool__st", "v_pool__sb", "v_pool__st"):
        assert call(**{field: 520}) == -1, field                     # 520 % 16 == 8
        assert call(**{field: 528}) == 0, field


def test_capability_and_workspace():
    lib = _lib.load()
    for fp8 in (0, 1):
        for dtype in (0, 1, 2):
            for hs, dv in ((32, 64), (64, 128), (128, 256)):
                for n in (1, 2, 3, 4):
                    for tq in range(1, 9):
                        assert lib.dta_decode_rows_supported(dtype, hs, n, dv, tq, fp8) == 1
            assert lib.dta_decode_rows_supported(dtype, 64, 1, 64, 8, fp8) == 1
            assert lib.dta_decode_rows_supported(dtype, 128, 1, 128, 8, fp8) == 1
            assert lib.dta_decode_rows_supported(dtype, 64, 2, 64, 2, fp8) == 0
            assert lib.dta_decode_rows_supported(dtype, 64, 2, 128, 0, fp8) == 0
            assert lib.dta_decode_rows_supported(dtype, 64, 2, 128, 9, fp8) == 0
            assert lib.dta_decode_rows_supported(dtype, 64, 5, 128, 2, fp8) == 0
            assert lib.dta_decode_rows_supported(dtype, 16, 2, 32, 2, fp8) == 0
        assert lib.dta_decode_rows_supported(3, 64, 2, 128, 2, fp8) == 0
    # the one-row split plan's partials and (max, sum) pairs, times the row count
    B, H, N, hs, dv = 3, 2, 2, 64, 128
    for t_cap in (1, 256, 257, 768, 32768):
        per_row = B * H * (-(-t_cap // 256)) * N * (dv + 2) * 4
        for tq in (1, 5, 8):
            assert lib.dta_attn_decode_rows_workspace_bytes(B, H, N, hs, dv, t_cap, tq) == tq * per_row
    # the one-row function is unchanged
    assert lib.dta_attn_decode_workspace_bytes(B, H, N, hs, dv, 768) == max(B * H * N * 768 * 4, B * H * 3 * N * (dv + 2) * 4)


# ----------------------------------------------------------------- dispatch ---
class _Cache:
    """Records which op ``_seq_attention_step`` asks the cache for."""
    kv_dtype = None
    fp8_extend = False

    def __init__(self, rows_decode):
        self.rows_decode = rows_decode
        self.calls = []

    def write_rows(self, layer, qkv, k_rot, dims, bs, tbl, pos, counts):
        return ()

    def _op(self, name, shape):
        self.calls.append(name)
        return torch.zeros(shape)

    def decode_rows(self, kv, q, coef, tbl, lengths):
        return self._op("decode", (q.shape[0], q.shape[1] * DV))

    def extend_rows(self, kv, q, coef, tbl, pos, counts):
        return self._op("extend", (q.shape[0], q.shape[1], q.shape[2] * DV))

    def rows_rows(self, kv, q, coef, tbl, pos, counts):
        return self._op("rows", (q.shape[0], q.shape[1], q.shape[2] * DV))


HN, NT, HS, DV = 2, 2, 64, 128


@pytest.fixture
def step(monkeypatch):
    """``_seq_attention_step`` with the model's pieces stubbed: a unit projection, no RoPE, no tail."""
    W = ops.packed_width(HN, NT, HS, DV)
    monkeypatch.setattr(kv_cache, "_spec", lambda block: (None, HN, NT, HS, DV, 64))
    monkeypatch.setattr(kv_cache, "_constants", lambda cache, attn, layer, H, hs, bs, x: (torch.zeros(W, 8), torch.ones(HN, NT), None))
    monkeypatch.setattr(kv_cache, "_attention_tail", lambda attn, out: out)
    plans = {"rows": True}
    monkeypatch.setattr(ops, "extend_supported", lambda *a: True)
    monkeypatch.setattr(ops, "decode_rows_supported", lambda dtype, hs, N, dv, Tq, fp8=False: plans["rows"] and 1 <= Tq <= 8)

    def run(cache, Tn, one_row=False):
        B = 3
        pos, counts = torch.tensor([5, 0, 9], dtype=torch.int32), torch.full((B,), Tn, dtype=torch.int32)
        rows = pos[:, None].long() + torch.arange(Tn)[None, :]
        out = kv_cache._seq_attention_step(None, torch.zeros(B, Tn, 8), 0, cache, None, pos, counts, rows, one_row)
        assert out.shape == (B, Tn, HN * DV)
        return cache.calls
    run.plans = plans
    return run


def test_the_flag_defaults_to_false():
    assert kv_cache.KVCache().rows_decode is False
    assert kv_cache.RaggedKVCache().rows_decode is False
    assert kv_cache.PagedKVCache(4, 32).rows_decode is False
    assert kv_cache.PagedKVCache(4, 32, kv_dtype="fp8_e4m3").rows_decode is False
    assert kv_cache.RaggedKVCache(rows_decode=True).rows_decode is True
    assert kv_cache.PagedKVCache(4, 32, rows_decode=True).rows_decode is True
    assert kv_cache.PagedKVCache(4, 32, kv_dtype="fp8_e4m3", rows_decode=True).fp8_extend is False


def test_dispatch_of_the_multi_row_step(step):
    for Tn in (2, 5, 8):
        assert step(_Cache(True), Tn) == ["rows"]
        assert step(_Cache(False), Tn) == ["extend"]                 # the default path does not move
    assert step(_Cache(True), 1, one_row=True) == ["decode"]         # the one-row step: the decode kernel
    assert step(_Cache(True), 1) == ["extend"]                       # a step one row wide is not a short multi-row step
    assert step(_Cache(True), 9) == ["extend"]                       # larger steps are not cut into groups of 8
    assert step(_Cache(True), 16) == ["extend"]
    step.plans["rows"] = False
    assert step(_Cache(True), 5) == ["extend"]                       # no plan: today's path


def test_fp8_pool_dispatch(step):
    cache = _Cache(True)
    cache.kv_dtype = "fp8_e4m3"
    assert step(cache, 4) == ["rows"]
    plain = _Cache(False)
    plain.kv_dtype = "fp8_e4m3"
    assert step(plain, 4) == ["decode"] * 4                          # the fp8 pool's default: one decode launch per row
    wide = _Cache(True)
    wide.kv_dtype = "fp8_e4m3"
    assert step(wide, 9) == ["decode"] * 9
