"""GPU checks of the multi-row step on the fp8 (e4m3fn) paged KV cache:
``dta_attn_extend_paged_fp8`` through ``ops.diff_attention_extend_paged_fp8`` and
``kv_cache.PagedKVCache(kv_dtype="fp8_e4m3", fp8_extend=True)``.

* Parity on a cache built by the torch reference quantiser, against
  ``oracle.diffattn_oracle.diff_core`` in fp32 on the dequantised rows with q rounded to its
  dtype (the comparison of test_gpu_fp8_cache._want).  x^ = byte * scale is exact in fp32; the
  only roundings are q, V^ and P to the operand type, the class of rounding
  test_extend_paged_matches_oracle_and_ragged_bitwise takes at test_gpu_ragged.TOL (1e-4 fp32,
  2e-2 bf16 / f16, conftest.rel_err), so that is the bar.  Every (row, head, branch) has its
  own magnitude, so an index mix-up between scales moves the result.  test_gpu_ragged.EXT_CASES:
  ragged positions and counts, a count of 0, a padded Tq of 33, one launch with counts=None.
  Pages shuffled; every byte and scale past a valid length and every unowned page poisoned
  (bytes 0x7F = NaN, scales NaN and +Inf alternating).
* Bitwise: placement of the pages, a sequence alone against the batch, counts=None against
  counts = Tq.
* Rows written by ``ops.kv_quant_rows`` and read back by the new op.
* Poisoned allocations and guard bands (tests/_poison.py): ``o`` is the only allocation.
* Model level: dispatch counted with a spy; one-layer fp32 models with and without the flag
  (cached bytes equal, logits to 1e-4: the two paths differ in fp32 summation order over the
  same dequantised values); two-layer models (layer 1's rows equal, the cache goes on working)."""
import functools

import pytest
import torch

import test_gpu_fp8_cache as F8
import test_gpu_paged as PG
import test_gpu_ragged as R
from _poison import poisoned_allocations
from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import ops, kv_cache

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = R.TOL
DTYPES = R.DTYPES
B, H = R.B, R.H
SHAPES = [(2, 64, 128), (2, 16, 32), (3, 64, 128), (1, 64, 64), (3, 128, 256)]
FP8 = "fp8_e4m3"
_i32 = R._i32


def _round_up(n, P):
    return -(-n // P) * P


def _counts(counts, Tq):
    return [Tq] * B if counts is None else list(counts)


@functools.lru_cache(maxsize=None)
def _inputs(N, hs, dv, case):
    """q, coef and the quantised cache rows of one EXT_CASES entry (host tensors), made once and shared."""
    pos, counts, Tq, cap = case
    g = torch.Generator().manual_seed(1000 * pos[1] + 13 * N + hs + dv + Tq)
    q = torch.randn(B, Tq, H, N, hs, generator=g)
    k = torch.randn(B, cap, H, N, hs, generator=g) * (0.25 + 2 * torch.rand(B, cap, H, N, 1, generator=g))
    v = torch.randn(B, cap, H, dv, generator=g) * (0.25 + 2 * torch.rand(B, cap, H, 1, generator=g))
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    kb, ks = ops.kv_quant_reference(k)
    vb, vs = ops.kv_quant_reference(v)
    return q, coef, kb, vb, torch.cat([ks, vs[..., None]], dim=-1)


def _oracle(q, k, v, coef, pos, n):
    """diff_core in fp32, per sequence: rows pos_b .. pos_b + n_b - 1 of the attention over its first
    pos_b + n_b rows; q (B, Tq, H, N, hs), k (B, >= L, H, N, hs), v (B, >= L, H, dv), all fp32 on the host."""
    Bn, Tq, Hn, N, hs = q.shape
    want = torch.zeros(Bn, Tq, Hn, v.shape[-1])
    for b in range(Bn):
        L = pos[b] + n[b]
        for h in range(Hn if n[b] else 0):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs)
                rows[0, pos[b]:] = q[b, :n[b], h, i]
                qs.append(rows)
            o = O.diff_core(qs, [k[b:b + 1, :L, h, i] for i in range(N)], v[b:b + 1, :L, h], coef[h])
            want[b, :n[b], h] = o[0, pos[b]:]
    return want


@functools.lru_cache(maxsize=None)
def _want(N, hs, dv, case, dtype):
    """The oracle on the dequantised rows, q as the kernel sees it (rounded to dtype)."""
    pos, counts, Tq, _ = case
    q, coef, kb, vb, sc = _inputs(N, hs, dv, case)
    k = kb.view(torch.float8_e4m3fn).float() * sc[..., :N, None]
    v = vb.view(torch.float8_e4m3fn).float() * sc[..., N, None]
    return _oracle(q.to(dtype).float(), k, v, coef, pos, _counts(counts, Tq))


def _check(got, want, n, Tq, dtype, dv, tag):
    assert got.shape == (B, Tq, H * dv) and got.dtype == dtype
    got = got.view(B, Tq, H, dv).float().cpu()
    assert torch.isfinite(got).all(), (tag, "poison reached the output")
    for b in range(B):
        assert (got[b, n[b]:] == 0).all(), (tag, b, "rows count_b .. are zeros")
        if n[b]:
            err = rel_err(got[b, :n[b]], want[b, :n[b]])
            print(f"extend_fp8 {tag} seq {b} count={n[b]}: rel_err {err:.3e} (bar {TOL[dtype]:.0e})")
            assert err <= TOL[dtype], (tag, b, err)


# ------------------------------------------------------------------ parity ---
@pytest.mark.parametrize("P", [32, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_extend_fp8_matches_the_oracle_on_dequantised_rows(dtype, N, hs, dv, P):
    assert ops.extend_fp8_supported(dtype, hs, N, dv)      # a missing plan cannot hide behind a fallback
    for case in R.EXT_CASES:
        pos, counts, Tq, cap0 = case
        q, coef, kb, vb, sc = _inputs(N, hs, dv, case)
        n = _counts(counts, Tq)
        valid = [pos[b] + n[b] for b in range(B)]
        k_pool, v_pool, scales, table = F8._paginate(kb, vb, sc, valid, P, _round_up(cap0, P), seed=P + Tq)
        got = ops.diff_attention_extend_paged_fp8(q.to(DEV, dtype), k_pool, v_pool, scales, coef.to(DEV), table,
                                                  _i32(pos), None if counts is None else _i32(counts))
        _check(got, _want(N, hs, dv, case, dtype), n, Tq, dtype, dv, (dtype, N, hs, dv, P, pos))


# ----------------------------------------------------------------- bitwise ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_extend_fp8_placement_and_batch_independence_bitwise(dtype):
    N, hs, dv, P = 2, 64, 128, 64
    case = R.EXT_CASES[0]
    pos, counts, Tq, cap0 = case
    q, coef, kb, vb, sc = _inputs(N, hs, dv, case)
    qd, cd = q.to(DEV, dtype), coef.to(DEV)
    valid = [p + c for p, c in zip(pos, counts)]
    cap = _round_up(cap0, P)
    outs = []
    for shuffle, seed in ((False, 0), (True, 1), (True, 2)):
        k_pool, v_pool, scales, table = F8._paginate(kb, vb, sc, valid, P, cap, seed=seed, shuffle=shuffle)
        outs.append(ops.diff_attention_extend_paged_fp8(qd, k_pool, v_pool, scales, cd, table, _i32(pos), _i32(counts)))
    assert torch.isfinite(outs[0].float()).all() and outs[0].abs().sum() > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for b in range(B):                                      # alone in the batch, a smaller pool
        k_pool, v_pool, scales, table = F8._paginate(kb[b:b + 1], vb[b:b + 1], sc[b:b + 1], valid[b:b + 1], P, cap,
                                                     seed=40 + b, spare=1)
        alone = ops.diff_attention_extend_paged_fp8(qd[b:b + 1], k_pool, v_pool, scales, cd, table, _i32(pos[b:b + 1]),
                                                    _i32(counts[b:b + 1]))
        assert torch.equal(outs[0][b:b + 1], alone), b


@pytest.mark.parametrize("dtype", DTYPES)
def test_extend_fp8_counts_none_is_counts_tq_bitwise(dtype):
    N, hs, dv, P = 2, 64, 128, 32
    case = R.EXT_CASES[2]
    pos, counts, Tq, cap0 = case
    assert counts is None
    q, coef, kb, vb, sc = _inputs(N, hs, dv, case)
    k_pool, v_pool, scales, table = F8._paginate(kb, vb, sc, [p + Tq for p in pos], P, _round_up(cap0, P), seed=7)
    args = (q.to(DEV, dtype), k_pool, v_pool, scales, coef.to(DEV), table, _i32(pos))
    none = ops.diff_attention_extend_paged_fp8(*args)
    full = ops.diff_attention_extend_paged_fp8(*args, _i32([Tq] * B))
    assert torch.isfinite(none.float()).all() and torch.equal(none, full)


# ---------------------------------------------------- write and read together ---
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", [(2, 64, 128), (3, 128, 256), (1, 64, 64)])
def test_rows_written_by_kv_quant_rows_are_read_back(dtype, N, hs, dv):
    P, n_pages, Tq = 32, 9, 5
    lens = [37, 5, 96]                                      # after the step; 37 and 96 end in their 2nd / 3rd page
    pos = [L - Tq for L in lens]
    Tn = max(lens)
    nq = H * N * hs
    g = torch.Generator().manual_seed(23 * N + hs)
    k_new = (torch.randn(B, Tn, H, N, hs, generator=g) * (0.25 + 2 * torch.rand(B, Tn, H, N, 1, generator=g))).to(DEV, dtype)
    v_new = (torch.randn(B, Tn, H, dv, generator=g) * (0.25 + 2 * torch.rand(B, Tn, H, 1, generator=g))).to(DEV, dtype)
    q = torch.randn(B, Tq, H, N, hs, generator=g)
    coef = torch.tensor([[1.0, -0.6, 0.3][:N]] * H)
    pool = torch.full((n_pages + 1, P, nq + H * dv), 0x7F, dtype=torch.uint8, device=DEV)
    scales = torch.full((n_pages + 1, P, H, N + 1), float("nan"), device=DEV)
    k_all, v_all = pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv))
    table = torch.tensor([[7, 2, -1], [4, -1, -1], [0, 8, 3]], dtype=torch.int32)
    t = torch.arange(Tn)
    slots = torch.stack([torch.where(t < lens[b], table[b].long().clamp(min=0)[(t // P).clamp(max=2)] * P + t % P,
                                     n_pages * P + t % P) for b in range(B)])       # padding rows: the spare page
    ops.kv_quant_rows(k_new, v_new, k_all, v_all, scales, slots.to(torch.int32).flatten().to(DEV))
    got = ops.diff_attention_extend_paged_fp8(q.to(DEV, dtype), k_all[:n_pages], v_all[:n_pages], scales[:n_pages],
                                              coef.to(DEV), table.to(DEV), _i32(pos))
    kd = torch.zeros(B, Tn, H, N, hs)
    vd = torch.zeros(B, Tn, H, dv)
    for b, L in enumerate(lens):
        kk, vv = ops.kv_dequant_reference(k_all[:n_pages], v_all[:n_pages], scales[:n_pages], table[b], L)
        kd[b, :L], vd[b, :L] = kk.cpu(), vv.cpu()
    assert torch.isfinite(kd).all() and torch.isfinite(vd).all()
    want = _oracle(q.to(dtype).float(), kd, vd, coef, pos, [Tq] * B)
    _check(got, want, [Tq] * B, Tq, dtype, dv, ("write+read", dtype, N, hs, dv))


# --------------------------------------------------- poisoned allocations ---
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", [(2, 64, 128), (3, 128, 256)])
def test_extend_fp8_poisoned_allocations(dtype, N, hs, dv):
    P, nq = 32, H * N * hs
    for case in R.EXT_CASES[:2]:
        pos, counts, Tq, cap0 = case
        q, coef, kb, vb, sc = _inputs(N, hs, dv, case)
        valid = [p + c for p, c in zip(pos, counts)]
        k_pool, v_pool, scales, table = F8._paginate(kb, vb, sc, valid, P, _round_up(cap0, P), seed=P + Tq)
        qd, cd, pd, cnt = q.to(DEV, dtype), coef.to(DEV), _i32(pos), _i32(counts)
        plain = ops.diff_attention_extend_paged_fp8(qd, k_pool, v_pool, scales, cd, table, pd, cnt)
        with poisoned_allocations() as s:
            pool = s.guarded(k_pool._base, "byte_pool")
            kp, vp = pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv))
            got = ops.diff_attention_extend_paged_fp8(s.guarded(qd, "q"), kp, vp, s.guarded(scales, "scale_pool"),
                                                      s.guarded(cd, "coef"), s.guarded(table, "block_table"),
                                                      s.guarded(pd, "pos"), s.guarded(cnt, "counts"))
            s.verify({"o"}, set())
        assert s.names() == ["o"]
        assert got.dtype == plain.dtype and torch.equal(got, plain), "the poisoned run differs from the plain run"
        _check(got, _want(N, hs, dv, case, dtype), list(counts), Tq, dtype, dv, ("poison", dtype, N, hs, dv, pos))


# ------------------------------------------------------------- model level ---
BS, P = PG.BS, PG.P
LENS = [30, 17, 60]                                         # + 5: 30 -> 35 and 60 -> 65 cross a page


@pytest.fixture
def spy(monkeypatch):
    calls = {"extend": 0, "decode": 0}
    ext, dec = ops.diff_attention_extend_paged_fp8, ops.diff_attention_decode_paged_fp8

    def extend(*a, **kw):
        calls["extend"] += 1
        return ext(*a, **kw)

    def decode(*a, **kw):
        calls["decode"] += 1
        return dec(*a, **kw)

    monkeypatch.setattr(ops, "diff_attention_extend_paged_fp8", extend)
    monkeypatch.setattr(ops, "diff_attention_decode_paged_fp8", decode)
    return calls


def _new_rows(seed=9):
    return torch.randint(0, 97, (3, 5), generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_dispatch_follows_the_flag(spy):
    model = PG._model("diff")
    layers = len(model.blocks)
    prompts, new = PG._prompts(8, LENS), _new_rows()
    for flag in (True, False):
        cache = kv_cache.PagedKVCache(12, P, kv_dtype=FP8, fp8_extend=flag)
        with torch.no_grad():
            ids, _ = kv_cache.prefill_paged(model, prompts, cache)
            assert spy == {"extend": 0, "decode": 0}        # the prefill runs the fused forward
            rows = kv_cache.append_paged(model, ids, new, [5, 5, 5], cache, all_rows=True)
            assert rows.shape == (3, 5, 97) and torch.isfinite(rows).all()
            assert spy == ({"extend": layers, "decode": 0} if flag else {"extend": 0, "decode": 5 * layers}), flag
            spy.update(extend=0, decode=0)
            kv_cache.decode_paged(model, ids, new[:, :1], cache)                 # the one-row step: the decode kernel
            assert spy == {"extend": 0, "decode": layers}, flag
            spy.update(extend=0, decode=0)


def test_dv_48_keeps_the_per_row_path(spy):
    torch.manual_seed(4)
    model = PG.C.StandardTransformer(97, 192, 4, 2, BS, 0.0).to(DEV).eval()      # hs = dv = 48, N = 1
    assert not ops.extend_fp8_supported(torch.float32, 48, 1, 48)
    prompts, new = PG._prompts(13, LENS), _new_rows(14)
    cache, plain = kv_cache.PagedKVCache(12, P, kv_dtype=FP8, fp8_extend=True), kv_cache.PagedKVCache(12, P, kv_dtype=FP8)
    with torch.no_grad():
        ids, _ = kv_cache.prefill_paged(model, prompts, cache)
        rows = kv_cache.append_paged(model, ids, new, [5, 5, 5], cache, all_rows=True)
        assert spy == {"extend": 0, "decode": 5 * len(model.blocks)}
        ids2, _ = kv_cache.prefill_paged(model, prompts, plain)
        want = kv_cache.append_paged(model, ids2, new, [5, 5, 5], plain, all_rows=True)
    assert rows.shape == (3, 5, 97) and torch.isfinite(rows).all()
    assert torch.equal(rows, want)                          # the flag changes nothing where there is no plan


def _one_layer(which):
    """The three models of test_gpu_paged with one layer, fp32."""
    if which == "diff":
        torch.manual_seed(0)
        model = PG.D.DiffTransformer(vocab_size=97, n_embd=256, n_head=2, n_layer=1, block_size=BS, dropout=0.0)
    elif which == "alt3":
        torch.manual_seed(1)
        model = PG.ND.AlternatingDiffTransformer(97, 256, 2, 1, BS, 0.0, n_terms=3)
    else:
        torch.manual_seed(2)
        model = PG.C.StandardTransformer(97, 256, 4, 1, BS, 0.0)
    model = model.to(DEV).eval()
    for p in model.parameters():          # non-zero lambdas so every branch weight differs
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model


def _raw_rows(cache, seq, layer):
    """The bytes (L, W) and scales (L, H * (N + 1)) of one sequence in one layer, as stored."""
    pages = torch.tensor(cache.pages[seq], device=DEV)
    L = cache.host_lengths[seq]
    return cache.pool[layer][pages].flatten(0, 1)[:L], cache.scale_pool[layer][pages].flatten(0, 1)[:L]


def _append_both(model, prompts, new):
    on, off = (kv_cache.PagedKVCache(12, P, kv_dtype=FP8, fp8_extend=flag) for flag in (True, False))
    with torch.no_grad():
        ids_on, a = kv_cache.prefill_paged(model, prompts, on)
        ids_off, b = kv_cache.prefill_paged(model, prompts, off)
        assert torch.equal(a, b)
        got = kv_cache.append_paged(model, ids_on, new, [5, 5, 5], on, all_rows=True)
        want = kv_cache.append_paged(model, ids_off, new, [5, 5, 5], off, all_rows=True)
    return on, off, ids_on, ids_off, got, want


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_one_layer_models_agree_with_the_per_row_path(which, spy):
    model = _one_layer(which)
    on, off, ids_on, ids_off, got, want = _append_both(model, PG._prompts(8, LENS), _new_rows())
    assert spy == {"extend": 1, "decode": 5}
    assert got.shape == want.shape == (3, 5, 97) and torch.isfinite(got).all()
    for q_on, q_off in zip(ids_on, ids_off):                # the writes see the same inputs
        (b_on, s_on), (b_off, s_off) = _raw_rows(on, q_on, 1), _raw_rows(off, q_off, 1)
        assert b_on.shape[0] == on.host_lengths[q_on] == off.host_lengths[q_off]
        assert torch.equal(b_on, b_off) and torch.equal(s_on, s_off), (which, q_on)
    for b in range(3):
        err = rel_err(got[b], want[b])
        print(f"one-layer {which} seq {b}: extend against per-row decode rel_err {err:.3e} (bar 1e-4)")
        assert err <= 1e-4, (which, b, err)


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_two_layer_models_run_and_the_cache_goes_on(which):
    model = PG._model(which)
    assert len(model.blocks) == 2
    on, off, ids_on, ids_off, got, want = _append_both(model, PG._prompts(8, LENS), _new_rows())
    assert got.shape == (3, 5, 97) and torch.isfinite(got).all()
    for q_on, q_off in zip(ids_on, ids_off):                # layer 1 sees embeddings only
        (b_on, s_on), (b_off, s_off) = _raw_rows(on, q_on, 1), _raw_rows(off, q_off, 1)
        assert torch.equal(b_on, b_off) and torch.equal(s_on, s_off), (which, q_on)
    assert [on.sync()[q] for q in ids_on] == [off.sync()[q] for q in ids_off] == [35, 22, 65]
    with torch.no_grad():
        on.truncate(ids_on[0], 31)                          # gives its second page back
        on.truncate(ids_on[2], 64)
        out = kv_cache.decode_paged(model, ids_on, _new_rows()[:, :1], on)
    assert out.shape == (3, 97) and torch.isfinite(out).all()
    assert [on.sync()[q] for q in ids_on] == [32, 23, 65]
