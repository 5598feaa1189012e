"""CPU checks of the fp8 (e4m3fn) paged KV cache: the two new entry points are in the
header and in the built library inside ABI 9, ``_lib.DecodePagedFp8Args`` /
``_lib.KvQuantRowsArgs`` lay their structs out as include/diffattn.h does (the gcc probe of
test_paged_cpu.py), the entry points reject bad arguments wherever they return before a
launch, the torch reference quantiser (``ops.kv_quant_reference``) meets its own error
bound, and ``kv_cache.PagedKVCache(kv_dtype="fp8_e4m3")`` keeps byte and scale pools of the
right shapes and copies both on write, with the model step stubbed so no kernel runs."""
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
    "dta_attn_decode_paged_fp8_args": _lib.DecodePagedFp8Args,
    "dta_kv_quant_rows_args": _lib.KvQuantRowsArgs,
}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_fp8_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    # the header declares both entry points with these signatures: sizeof of a call is not
    # evaluated, so nothing links, and an undeclared or differently typed function does not compile
    lines += ['  printf("symbols declared %zu\\n", sizeof(dta_attn_decode_paged_fp8((const dta_attn_decode_paged_fp8_args*)0, (void*)0))'
              ' / sizeof(dta_kv_quant_rows((const dta_kv_quant_rows_args*)0, (void*)0)));',
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
    # the fp8 decode struct is the paged one with the scale pool appended
    assert ([f[0] for f in _lib.DecodePagedArgs._fields_] + ["scale_pool_dev", "scale_page_stride"]
            == [f[0] for f in _lib.DecodePagedFp8Args._fields_])


def _decode_args(**kw):
    """An fp8 paged decode call that passes every host check at B = 0, so no pointer is
    dereferenced and nothing is launched (the scheme of test_paged_cpu._decode_args)."""
    a = _lib.DecodePagedFp8Args()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 2, 2, 64, 128
    a.length, a.t_cap, a.scale = 8, 128, 0.125
    a.page_size, a.max_pages, a.n_pages = 64, 2, 4
    buf = (ctypes.c_int32 * 8)()
    a.lengths_dev = ctypes.addressof(buf)
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


def _quant_args(**kw):
    a = _lib.KvQuantRowsArgs()
    a.dtype, a.B, a.Tn, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 3, 2, 2, 64, 128
    a.page_size, a.n_pages = 64, 4
    buf = (ctypes.c_int32 * 8)()
    a.slot_dev = ctypes.addressof(buf)
    a.scale_pool_dev = ctypes.addressof(buf)
    a.scale_page_stride = 64 * 2 * 3
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_fp8_entry_points_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    for name in _lib.FP8_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.FP8_EXPORTS == ("dta_attn_decode_paged_fp8", "dta_kv_quant_rows")
    assert ops.fp8_cache_supported() is True

    class _Old:                                   # a library of the same ABI without the symbols
        dta_attn_decode_paged = dta_attn_extend_paged = None
    assert not _lib.fp8_symbols(_Old())

    dec = lib.dta_attn_decode_paged_fp8
    assert dec(None, None) == -1
    assert dec(ctypes.byref(_lib.DecodePagedFp8Args()), None) == -1
    assert dec(ctypes.byref(_decode_args()), None) == 0                               # B = 0: valid, no launch
    # everything dta_attn_decode_paged rejects
    assert dec(ctypes.byref(_decode_args(page_size=32, max_pages=4, scale_page_stride=32 * 6)), None) == 0
    assert dec(ctypes.byref(_decode_args(page_size=256, max_pages=1, t_cap=256, scale_page_stride=256 * 6)), None) == 0
    assert dec(ctypes.byref(_decode_args(page_size=48, max_pages=2, t_cap=96)), None) == -1
    assert dec(ctypes.byref(_decode_args(page_size=512, max_pages=1, t_cap=512, scale_page_stride=512 * 6)), None) == -1
    assert dec(ctypes.byref(_decode_args(t_cap=127)), None) == -1
    assert dec(ctypes.byref(_decode_args(max_pages=3)), None) == -1
    assert dec(ctypes.byref(_decode_args(block_table_dev=None)), None) == -1
    assert dec(ctypes.byref(_decode_args(block_table_dev=_decode_args().block_table_dev + 2)), None) == -1
    assert dec(ctypes.byref(_decode_args(n_pages=0)), None) == -1
    assert dec(ctypes.byref(_decode_args(lengths_dev=None)), None) == -1
    assert dec(ctypes.byref(_decode_args(lengths_dev=_decode_args().lengths_dev + 1)), None) == -1
    assert dec(ctypes.byref(_decode_args(dtype=3)), None) == -1
    assert dec(ctypes.byref(_decode_args(length=0)), None) == -1
    assert dec(ctypes.byref(_decode_args(length=129)), None) == -1                    # > t_cap
    assert dec(ctypes.byref(_decode_args(head_size=132)), None) == -2
    assert dec(ctypes.byref(_decode_args(n_terms=5, scale_page_stride=64 * 2 * 6)), None) == -2
    assert dec(ctypes.byref(_decode_args(dv=264)), None) == -2
    # the fp8 arguments
    assert dec(ctypes.byref(_decode_args(scale_pool_dev=None)), None) == -1
    assert dec(ctypes.byref(_decode_args(scale_pool_dev=_decode_args().scale_pool_dev + 2)), None) == -1
    assert dec(ctypes.byref(_decode_args(scale_page_stride=64 * 2 * 3 - 1)), None) == -1
    assert dec(ctypes.byref(_decode_args(scale_page_stride=64 * 2 * 3 + 5)), None) == 0      # padding between pages is fine
    for field in ("k_pool__sb", "k_pool__st", "v_pool__sb", "v_pool__st"):
        assert dec(ctypes.byref(_decode_args(**{field: 520})), None) == -1, field            # 520 % 16 == 8
        assert dec(ctypes.byref(_decode_args(**{field: 528})), None) == 0, field

    qnt = lib.dta_kv_quant_rows
    assert qnt(None, None) == -1
    assert qnt(ctypes.byref(_lib.KvQuantRowsArgs()), None) == -1
    assert qnt(ctypes.byref(_quant_args()), None) == 0                                # B = 0: valid, no launch
    assert qnt(ctypes.byref(_quant_args(Tn=0, B=2)), None) == 0
    for bad in (dict(head_size=40, dv=80), dict(head_size=72), dict(dv=136), dict(n_terms=5, scale_page_stride=64 * 2 * 6),
                dict(head_size=144), dict(dv=272)):
        assert qnt(ctypes.byref(_quant_args(**bad)), None) == -2, bad
    for bad in (dict(dtype=3), dict(n_terms=0), dict(page_size=48), dict(page_size=16), dict(n_pages=0),
                dict(slot_dev=None), dict(slot_dev=_quant_args().slot_dev + 2), dict(scale_pool_dev=None),
                dict(scale_pool_dev=_quant_args().scale_pool_dev + 1), dict(scale_page_stride=64 * 2 * 3 - 1), dict(B=-1)):
        assert qnt(ctypes.byref(_quant_args(**bad)), None) == -1, bad


# ------------------------------------------------------- reference quantiser ---
def _bound(x, scale):
    """|x^ - x| <= 2^-4 |x| + 2^-10 scale: half a step of 3 mantissa bits, and half the
    subnormal step (2^-9 in units of the scale)."""
    return x.abs() * 2.0 ** -4 + scale[..., None] * 2.0 ** -10


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_quantiser_meets_its_bound(dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 5, 64, generator=g) * torch.logspace(-3, 2, 7)[:, None, None]
    x[0, 0] = 0.0                                              # a zero vector
    x[1, 1, :60] *= 1e-3                                       # a few large values, the rest in the subnormal range
    x[2, 2, 5] = 500.0 * x[2, 2].abs().max()                   # an outlier 500 x the rest
    x = x.to(dtype)
    byte, scale = ops.kv_quant_reference(x)
    assert byte.dtype == torch.uint8 and byte.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    xf = x.float()
    amax = xf.abs().amax(-1)
    assert torch.equal(scale, amax / 448.0)
    deq = byte.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(deq).all()                            # no NaN byte (0x7f / 0xff), whatever the outlier
    assert (byte & 0x7F != 0x7F).all()
    xhat = deq * scale[..., None]
    assert (xhat - xf).abs().le(_bound(xf, scale)).all()
    # the element of largest magnitude maps to +-448 exactly
    top = xf.abs().argmax(-1, keepdim=True)
    assert torch.equal(deq.gather(-1, top)[amax > 0].abs(), torch.full_like(amax[amax > 0], 448.0)[:, None])
    assert torch.equal(deq.gather(-1, top).sign(), xf.gather(-1, top).sign())
    # a zero vector: scale 0 and bytes 0
    assert scale[0, 0] == 0 and (byte[0, 0] == 0).all()
    # torch's own conversion does not saturate: the clamp in the reference is what keeps 500 finite
    assert torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all()
    y = torch.tensor([[500.0, 1.0]])
    b2, s2 = ops.kv_quant_reference(y)
    assert torch.equal(b2.view(torch.float8_e4m3fn).float()[0, 0], torch.tensor(448.0))


def test_dequant_reference_gathers_through_the_table():
    g = torch.Generator().manual_seed(4)
    n_pages, P, H, N, hs, dv = 5, 32, 2, 2, 16, 32
    k = torch.randn(n_pages, P, H, N, hs, generator=g)
    v = torch.randn(n_pages, P, H, dv, generator=g)
    kb, ks = ops.kv_quant_reference(k)
    vb, vs = ops.kv_quant_reference(v)
    scales = torch.cat([ks, vs[..., None]], dim=-1)
    table = [3, 0, 4, -1]
    kd, vd = ops.kv_dequant_reference(kb, vb, scales, table, 70)
    assert kd.shape == (70, H, N, hs) and vd.shape == (70, H, dv)
    want_k = torch.cat([k[3], k[0], k[4]])[:70]
    want_v = torch.cat([v[3], v[0], v[4]])[:70]
    assert (kd - want_k).abs().le(_bound(want_k, torch.cat([ks[3], ks[0], ks[4]])[:70])).all()
    assert (vd - want_v).abs().le(_bound(want_v, torch.cat([vs[3], vs[0], vs[4]])[:70])).all()


# ------------------------------------------------------------------- cache ---
class _Model:
    block_size = 256


P, POOL = 32, 12


@pytest.fixture
def calls(monkeypatch):
    out = []

    def step(model, idx, cache, tbl, pos, counts, gather=None, one_row=False):
        out.append(tuple(idx.shape))
        if gather is None:
            return torch.zeros(idx.shape[0], idx.shape[1], 3)
        return torch.zeros(idx.shape[0], 3)

    monkeypatch.setattr(kv_cache, "_paged_model_step", step)
    return out


def _prompts(*lens):
    return [torch.arange(n, dtype=torch.long) % 5 for n in lens]


def test_fp8_cache_pools_bytes_and_copy_on_write(calls):
    H, N, hs, dv = 16, 2, 64, 128
    W = H * N * hs + H * dv
    model = _Model()
    cache = kv_cache.PagedKVCache(POOL, P, kv_dtype="fp8_e4m3")
    plain = kv_cache.PagedKVCache(POOL, P)
    assert cache.kv_dtype == "fp8_e4m3" and plain.kv_dtype is None and plain.scale_pool == {}
    for layer in (1, 2):
        pool, scales = cache.layer_pool_fp8(layer, W, H, N, "cpu")
        assert pool.dtype == torch.uint8 and pool.shape == (POOL + 1, P, W)
        assert scales.dtype == torch.float32 and scales.shape == (POOL + 1, P, H * (N + 1))
        assert cache.layer_pool_fp8(layer, W, H, N, "cpu")[0] is pool                # made once
        plain.layer_pool(layer, W, torch.zeros(1, dtype=torch.bfloat16))
    # bytes per (row, head): N*hs + dv + 4*(N+1) = 268 against 2*(N*hs + dv) = 512
    assert cache.cache_bytes() * 512 == plain.cache_bytes() * 268
    assert cache.cache_bytes() == 2 * (POOL + 1) * P * H * 268

    (a,), _ = kv_cache.prefill_paged(model, _prompts(40), cache)
    for layer in (1, 2):
        cache.pool[layer].copy_((torch.arange(cache.pool[layer].numel()) % 251).view_as(cache.pool[layer]) + layer)
        cache.scale_pool[layer].copy_(torch.arange(cache.scale_pool[layer].numel()).view_as(cache.scale_pool[layer]) + 0.5 * layer)
    before = {layer: (cache.pool[layer].clone(), cache.scale_pool[layer].clone()) for layer in (1, 2)}
    c = cache.fork(a)
    old = cache.pages[a][1]
    kv_cache.append_paged(model, [c], torch.zeros(1, 2, dtype=torch.long), [2], cache)
    new = cache.pages[c][1]
    assert new != old and cache.pages[a][1] == old and cache.pages[c][0] == cache.pages[a][0]
    for layer in (1, 2):
        assert torch.equal(cache.pool[layer][new], before[layer][0][old])            # the bytes ...
        assert torch.equal(cache.scale_pool[layer][new], before[layer][1][old])      # ... and their scales, same page ids
        keep = [pg for pg in range(POOL + 1) if pg != new]
        assert torch.equal(cache.pool[layer][keep], before[layer][0][keep])
        assert torch.equal(cache.scale_pool[layer][keep], before[layer][1][keep])
    cache.release(c)
    cache.truncate(a, 3)
    assert cache.pages_in_use() == 1


def test_bad_kv_dtype_raises(calls):
    for bad in ("fp8", "e5m2", "bf16", torch.float8_e4m3fn, 8):
        with pytest.raises(ValueError):
            kv_cache.PagedKVCache(POOL, P, kv_dtype=bad)
        with pytest.raises(ValueError):
            kv_cache.generate_paged(_Model(), _prompts(3), 2, kv_dtype=bad)
    assert calls == []
    out = kv_cache.generate_paged(_Model(), _prompts(3), 0, kv_dtype="fp8_e4m3")
    assert [o.tolist() for o in out] == [[0, 1, 2]]
