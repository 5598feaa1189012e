"""GPU parity of the multi-row step over the KV cache (``dta_attn_extend``).

* ``ops.diff_attention_extend`` against the oracle's ``diff_core`` (the reference's
  combine-then-@V, diff_transformer.py:57-72 / Ndiff_transformer.py:102-125) in fp64
  on the CPU: Tq query rows at positions pos .. pos+Tq-1 must equal rows ``pos:`` of
  the full causal attention over the same pos+Tq positions -- with the cache tail
  random, and poisoned with NaN.
* Agreement with the training forward (``dta_attn_fwd``) and the one-row decode
  (``dta_attn_decode``) on the strided views of one packed projection output.
* The argument contract of the op.
* Model level: ``kv_cache.append_logits`` (every row's logits) and the chunked
  prefill (``prefill_chunk``) against a full forward of the same window, for
  DiffTransformer, AlternatingDiffTransformer (RoPE rows) and control.py's
  StandardTransformer; single-token decode goes on afterwards, graph and eager.
* The per-row decode fallback for a head size without an extend plan (40).
Tolerances (north_star): fp32 max|a-b|/max|b| <= 1e-4, bf16 / f16 <= 2e-2.
"""
import functools

import pytest
import torch

from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import ops, kv_cache
from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import Ndiff_transformer as ND
from differential_transformer_replication_amd import control as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 2e-2}
B, H = 2, 3

SHAPES = [(1, 64, 64), (2, 16, 32), (2, 32, 64), (2, 64, 128), (3, 64, 128), (4, 32, 64), (2, 96, 192),
          (2, 128, 256), (8, 16, 32)]
# (pos, Tq, cap): pos = 0; a single row; query / key tiles that are partial and straddle
# a multiple of 32; a diagonal tile at an unaligned pos
CASES = [(0, 1, 1), (0, 33, 40), (5, 3, 9), (31, 2, 64), (32, 32, 64), (63, 70, 160), (200, 57, 300)]
POISON_CASES = [(63, 70, 160), (5, 3, 9)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _case(N, hs, dv, pos, Tq, cap):
    """CPU inputs and the fp64 oracle rows pos .. pos+Tq-1, computed once per case and
    shared (read-only) by the dtype and poison variants."""
    g = torch.Generator().manual_seed(1000 * pos + 7 * N + hs + Tq)
    L = pos + Tq
    q = torch.randn(B, cap, H, N, hs, generator=g)
    k = torch.randn(B, cap, H, N, hs, generator=g)
    v = torch.randn(B, cap, H, dv, generator=g)
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    want = torch.empty(B, Tq, H, dv, dtype=torch.float64)
    for h in range(H):
        o = O.diff_core([q[:, :L, h, i].double() for i in range(N)], [k[:, :L, h, i].double() for i in range(N)],
                        v[:, :L, h].double(), coef[h].double())
        want[:, :, h] = o[:, pos:]
    return q, k, v, coef, want


def _run(dtype, N, hs, dv, pos, Tq, cap, poison=False):
    q, k, v, coef, want = _case(N, hs, dv, pos, Tq, cap)
    qd, kd, vd = (t.to(DEV, dtype) for t in (q, k, v))
    if poison:
        kd[:, pos + Tq:] = float("nan")
        vd[:, pos + Tq:] = float("nan")
    got = ops.diff_attention_extend(qd[:, pos:pos + Tq], kd, vd, coef.to(DEV), pos)
    assert got.shape == (B, Tq, H * dv) and got.dtype == dtype
    return got.view(B, Tq, H, dv).float(), want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_extend_kernel_matches_oracle(dtype, N, hs, dv):
    assert ops.extend_supported(dtype, hs, N, dv)          # a missing plan cannot hide behind a fallback
    for pos, Tq, cap in CASES:
        got, want = _run(dtype, N, hs, dv, pos, Tq, cap)
        err = rel_err(got, want)
        print(f"extend {dtype} N={N} hs={hs} dv={dv} pos={pos} Tq={Tq} cap={cap}: rel_err {err:.3e}")
        assert err <= TOL[dtype], (dtype, N, hs, dv, pos, Tq, cap)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_extend_ignores_poisoned_cache_tail(dtype, N, hs, dv):
    """KVCache.layer allocates with torch.empty: rows >= pos+Tq may hold NaN."""
    for pos, Tq, cap in POISON_CASES:
        got, want = _run(dtype, N, hs, dv, pos, Tq, cap, poison=True)
        assert torch.isfinite(got).all(), (dtype, N, hs, dv, pos, Tq)
        assert rel_err(got, want) <= TOL[dtype], (dtype, N, hs, dv, pos, Tq, cap)


def test_extend_matches_fused_forward_and_decode():
    """Same packed qkv through dta_attn_fwd (T = L), dta_attn_decode and dta_attn_extend,
    on the strided split_packed views."""
    Bq, Hq, N, hs, L = 2, 4, 2, 64, 384
    dv = 2 * hs
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(Bq, L, ops.packed_width(Hq, N, hs, dv), generator=g).to(DEV)
    coef = torch.tensor([[1.0, -0.6]] * Hq, device=DEV)
    with torch.no_grad():
        full = ops.diff_attention(qkv, coef, Hq, N, hs)
    q, k, v = ops.split_packed(qkv, Hq, N, hs, dv)
    assert not k.is_contiguous() and not v.is_contiguous()
    ext = ops.diff_attention_extend(q[:, L - 40:], k, v, coef, L - 40)
    assert rel_err(ext, full[:, L - 40:]) <= 1e-4
    one = ops.diff_attention_extend(q[:, L - 1:], k, v, coef, L - 1)
    dec = ops.diff_attention_decode(q[:, -1], k, v, coef, L)
    assert rel_err(one[:, 0], dec) <= 1e-4


def test_extend_contract():
    q = torch.zeros(1, 4, 1, 2, 64, device=DEV)
    k = torch.zeros(1, 8, 1, 2, 64, device=DEV)
    v = torch.zeros(1, 8, 1, 128, device=DEV)
    coef = torch.ones(1, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ops.diff_attention_extend(q, k, v, coef, 5)                  # pos + Tq > cap
    with pytest.raises(RuntimeError):
        ops.diff_attention_extend(q, k, v, coef, -1)
    assert not ops.extend_supported(torch.float32, 40, 2, 80)
    with pytest.raises(RuntimeError):
        ops.diff_attention_extend(torch.zeros(1, 4, 1, 2, 40, device=DEV), torch.zeros(1, 8, 1, 2, 40, device=DEV),
                                  torch.zeros(1, 8, 1, 80, device=DEV), coef, 0)
    out = ops.diff_attention_extend(q[:, :0], k, v, coef, 3)         # Tq = 0
    assert out.shape == (1, 0, 128)


# ------------------------------------------------------------- model level ---
def _models():
    torch.manual_seed(0)
    yield "diff", D.DiffTransformer(vocab_size=97, n_embd=256, n_head=2, n_layer=2, block_size=24, dropout=0.0)
    torch.manual_seed(1)
    yield "alt3", ND.AlternatingDiffTransformer(97, 256, 2, 2, 24, 0.0, n_terms=3)
    torch.manual_seed(2)
    yield "ctrl", C.StandardTransformer(97, 256, 4, 2, 24, 0.0)        # N = 1, dv = hs = 64, RoPE


def _model(which):
    model = dict(_models())[which].to(DEV).eval()
    for p in model.parameters():          # non-zero lambdas so every branch weight differs
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_append_logits_match_full_forward(which, graph, monkeypatch):
    monkeypatch.setenv("DTA_DECODE_GRAPH", graph)
    model = _model(which)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 97, (2, 7), generator=g).to(DEV)
    cache = kv_cache.KVCache()
    with torch.no_grad():
        got = kv_cache.last_logits(model, idx, cache)
        assert rel_err(got, model(idx)[0][:, -1]) <= 1e-4
        new = torch.randint(0, 97, (2, 5), generator=g).to(DEV)
        rows = kv_cache.append_logits(model, new, cache, all_rows=True)
        idx = torch.cat([idx, new], dim=1)
        assert rows.shape == (2, 5, 97) and cache.length == 12
        assert rel_err(rows, model(idx)[0][:, -5:]) <= 1e-4, which
        for step in range(3):                                # single-token decode goes on
            idx = torch.cat([idx, torch.randint(0, 97, (2, 1), generator=g).to(DEV)], dim=1)
            got = kv_cache.last_logits(model, idx, cache)
            assert rel_err(got, model(idx)[0][:, -1]) <= 1e-4, (which, graph, step)
        assert cache.length == 15
        last = kv_cache.append_logits(model, new[:, :2], cache)       # last row only
        idx = torch.cat([idx, new[:, :2]], dim=1)
        assert last.shape == (2, 97)
        assert rel_err(last, model(idx)[0][:, -1]) <= 1e-4
        with pytest.raises(ValueError):
            kv_cache.append_logits(model, torch.zeros(2, 8, dtype=torch.long, device=DEV), cache)   # 17 + 8 > 24


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_append_logits_bf16_autocast(which):
    model = _model(which)
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, 97, (2, 12), generator=g).to(DEV)
    cache = kv_cache.KVCache()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        kv_cache.last_logits(model, idx[:, :7], cache)
        rows = kv_cache.append_logits(model, idx[:, 7:], cache, all_rows=True)
        want = model(idx)[0][:, -5:]
    assert rel_err(rows.float(), want.float()) <= 2e-2


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_chunked_prefill_matches_full_forward(which):
    model = _model(which)
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, 97, (2, 11), generator=g).to(DEV)
    cache = kv_cache.KVCache()
    with torch.no_grad():
        got = kv_cache.prefill_logits(model, idx, cache, prefill_chunk=4)      # rows 4 + 4 + 3
        assert cache.length == 11
        assert rel_err(got, model(idx)[0][:, -1]) <= 1e-4, which
        idx2 = torch.cat([idx, torch.randint(0, 97, (2, 1), generator=g).to(DEV)], dim=1)
        nxt = kv_cache.last_logits(model, idx2, cache)                          # decode on the chunked cache
        assert cache.length == 12
        assert rel_err(nxt, model(idx2)[0][:, -1]) <= 1e-4, which
        out = model.generate(idx, 6, prefill_chunk=4)
    assert out.shape == (2, 17)
    assert torch.equal(out[:, :11], idx)
    with pytest.raises(ValueError):
        model.generate(idx, 1, prefill_chunk=0)


def test_append_fallback_loop_head_size_40():
    """hs = 40 has no extend plan: the multi-row step runs one decode launch per row."""
    torch.manual_seed(4)
    model = C.StandardTransformer(97, 160, 4, 2, 24, 0.0).to(DEV).eval()      # hs = dv = 40, N = 1
    assert not ops.extend_supported(torch.float32, 40, 1, 40)
    g = torch.Generator().manual_seed(13)
    idx = torch.randint(0, 97, (2, 12), generator=g).to(DEV)
    cache = kv_cache.KVCache()
    with torch.no_grad():
        kv_cache.last_logits(model, idx[:, :7], cache)
        rows = kv_cache.append_logits(model, idx[:, 7:], cache, all_rows=True)
        want = model(idx)[0][:, -5:]
    assert rel_err(rows, want) <= 1e-4
