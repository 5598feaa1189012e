"""GPU checks of the fp8 (e4m3fn) paged KV cache: ``dta_attn_decode_paged_fp8`` and
``dta_kv_quant_rows`` through ``ops`` and ``kv_cache``.

* Decode parity on a cache built by the torch reference quantiser (so the write kernel is
  not part of it), against ``oracle.diffattn_oracle.diff_core`` in fp32 on the dequantised
  rows.  x^ = byte * scale is exact in fp32 and the kernel accumulates in fp32 as the
  16-bit one does, so quantisation error is not in this comparison and the tolerance is
  test_gpu_ragged.TOL for the dtype of q (1e-4 fp32, 2e-2 bf16 / f16, conftest.rel_err).
  Pages shuffled; every byte and scale past a length and every unowned page poisoned
  (bytes 0x7F = NaN, scales NaN and +Inf); a length of 0 gives zeros.
* The 512-key chunk plan, placement independence (bitwise).
* The write kernel against the quantiser's own bound, element by element:
  |x^ - x| <= 2^-4 |x| + 2^-10 scale (half a step of 3 mantissa bits, half the subnormal
  step) plus one fp32 ulp of x / scale, in units of the scale, of slack; scales within 1e-6
  of amax / 448; the amax element exactly +-448; nothing but the named rows changes.
* Model level (the three models of test_gpu_paged): cached rows of every layer against an
  unquantised twin, continuous batching, fork with copy on write of the scale pages,
  append against one-at-a-time decode, generate_paged(kv_dtype=...)."""
import functools

import pytest
import torch

import test_gpu_paged as PG
import test_gpu_ragged as R
from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import ops, kv_cache

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = R.TOL
DTYPES = R.DTYPES
B, H = 3, 2
CAP = 1024
LENGTHS = [(1, 255, 256), (257, 600, 0)]          # {1, 255, 256, 257, 600, 0} spread over the batch
SPLIT_SHAPES = [(2, 32, 64), (2, 64, 128), (1, 64, 64), (3, 128, 256)]
SHAPES = SPLIT_SHAPES + [(2, 40, 80)]             # the last one: no split plan, the single-pass kernel
FP8 = "fp8_e4m3"


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _inputs(N, hs, dv):
    """q, coef and the quantised cache rows (host tensors), made once per shape and shared."""
    g = torch.Generator().manual_seed(13 * N + hs + dv)
    q = torch.randn(B, H, N, hs, generator=g)
    k = torch.randn(B, 600, H, N, hs, generator=g) * (0.25 + 2 * torch.rand(B, 600, H, N, 1, generator=g))
    v = torch.randn(B, 600, H, dv, generator=g) * (0.25 + 2 * torch.rand(B, 600, H, 1, generator=g))
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    kb, ks = ops.kv_quant_reference(k)
    vb, vs = ops.kv_quant_reference(v)
    return q, coef, kb, vb, torch.cat([ks, vs[..., None]], dim=-1)


@functools.lru_cache(maxsize=None)
def _want(N, hs, dv, lengths, dtype):
    """diff_core in fp32 on the dequantised rows, q as the kernel sees it (rounded to dtype)."""
    q, coef, kb, vb, sc = _inputs(N, hs, dv)
    q = q.to(dtype).float()
    k = kb.view(torch.float8_e4m3fn).float() * sc[..., :N, None]
    v = vb.view(torch.float8_e4m3fn).float() * sc[..., N, None]
    want = torch.zeros(B, H, dv)
    for b, L in enumerate(lengths):
        for h in range(H if L else 0):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs)
                rows[0, -1] = q[b, h, i]
                qs.append(rows)
            want[b, h] = O.diff_core(qs, [k[b:b + 1, :L, h, i] for i in range(N)], v[b:b + 1, :L, h], coef[h])[0, -1]
    return want


def _paginate(kb, vb, sc, valid, P, cap, seed, spare=5, shuffle=True):
    """Cut the quantised rows (B, T, ...) into pages over a packed byte pool and a scale
    pool, by a fixed random permutation (or in order); everything past valid[b] and every
    unowned page is poison: bytes 0x7F (NaN in e4m3fn), scales NaN and +Inf alternating."""
    Bn, _, Hn, N, hs = kb.shape
    dv = vb.shape[-1]
    nq = Hn * N * hs
    max_pages = cap // P
    n_pages = Bn * max_pages + spare
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)) if shuffle else torch.arange(n_pages)
    perm = order[:Bn * max_pages].view(Bn, max_pages)
    pool = torch.full((n_pages, P, nq + Hn * dv), 0x7F, dtype=torch.uint8)
    scales = torch.full((n_pages, P, Hn, N + 1), float("nan"))
    scales.view(-1)[::2] = float("inf")
    table = torch.full((Bn, max_pages), -1, dtype=torch.int32)
    for b, L in enumerate(valid):
        for p in range(-(-L // P)):
            n = min(P, L - p * P)
            table[b, p] = perm[b, p]
            pool[perm[b, p], :n, :nq] = kb[b, p * P:p * P + n].flatten(1)
            pool[perm[b, p], :n, nq:] = vb[b, p * P:p * P + n].flatten(1)
            scales[perm[b, p], :n] = sc[b, p * P:p * P + n]
    pool, scales = pool.to(DEV), scales.to(DEV)
    return pool[..., :nq].unflatten(-1, (Hn, N, hs)), pool[..., nq:].unflatten(-1, (Hn, dv)), scales, table.to(DEV)


# ------------------------------------------------------------------ decode ---
@pytest.mark.parametrize("P", [32, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_decode_fp8_matches_the_oracle_on_dequantised_rows(dtype, N, hs, dv, P):
    q, coef, kb, vb, sc = _inputs(N, hs, dv)
    qd, cd = q.to(DEV, dtype), coef.to(DEV)
    for lengths in LENGTHS:
        k_pool, v_pool, scales, table = _paginate(kb, vb, sc, lengths, P, CAP, seed=P + sum(lengths))
        got = ops.diff_attention_decode_paged_fp8(qd, k_pool, v_pool, scales, cd, table, _i32(lengths))
        assert got.shape == (B, H * dv) and got.dtype == dtype
        tight = ops.diff_attention_decode_paged_fp8(qd, k_pool, v_pool, scales, cd, table, _i32(lengths),
                                                    max(max(lengths), 1))
        assert torch.equal(tight, got), (dtype, N, hs, P, lengths, "max_length moved the result")
        got = got.view(B, H, dv).float().cpu()
        assert torch.isfinite(got).all(), (dtype, N, hs, P, lengths, "poison reached the output")
        want = _want(N, hs, dv, lengths, dtype)
        for b, L in enumerate(lengths):
            if L == 0:
                assert (got[b] == 0).all(), (dtype, N, hs, P, "an empty sequence writes zeros")
            else:
                err = rel_err(got[b], want[b])
                print(f"decode_fp8 {dtype} N={N} hs={hs} dv={dv} P={P} len={L}: rel_err {err:.3e}")
                assert err <= TOL[dtype], (dtype, N, hs, dv, P, lengths, b)


def test_decode_fp8_wide_chunk_plan():
    """ceil(t_cap / 256) * H * B >= 8192: the 512-key chunk plan, as
    test_decode_paged_wide_chunk_plan_bitwise builds it; lengths 511, 513 and 0."""
    Bw, Hw, N, hs, dv, P, cap = 8, 16, 2, 32, 64, 64, 16384
    assert -(-cap // 256) * Hw * Bw >= 8192
    lengths = [511, 513, 0, 511, 513, 0, 513, 511]
    g = torch.Generator().manual_seed(5)
    q = torch.randn(Bw, Hw, N, hs, generator=g)
    coef = torch.tensor([[1.0, -0.6]] * Hw)
    kb, ks = ops.kv_quant_reference(torch.randn(3, 513, Hw, N, hs, generator=g))
    vb, vs = ops.kv_quant_reference(torch.randn(3, 513, Hw, dv, generator=g))
    sc = torch.cat([ks, vs[..., None]], dim=-1)
    pick = [b % 3 for b in range(Bw)]
    k_pool, v_pool, scales, table = _paginate(kb[pick], vb[pick], sc[pick], lengths, P, 576, seed=6)
    table = torch.cat([table, torch.full((Bw, cap // P - table.shape[1]), -1, dtype=torch.int32, device=DEV)], dim=1)
    got = ops.diff_attention_decode_paged_fp8(q.to(DEV, torch.bfloat16), k_pool, v_pool, scales, coef.to(DEV),
                                              table.contiguous(), _i32(lengths))
    got = got.view(Bw, Hw, dv).float().cpu()
    assert torch.isfinite(got).all()
    qf = q.to(torch.bfloat16).float()
    for b, L in enumerate(lengths):
        if L == 0:
            assert (got[b] == 0).all()
            continue
        k = kb[pick[b], :L].view(torch.float8_e4m3fn).float() * sc[pick[b], :L, :, :N, None]
        v = vb[pick[b], :L].view(torch.float8_e4m3fn).float() * sc[pick[b], :L, :, N, None]
        s = torch.einsum("hid,lhid->hil", qf[b], k) / hs ** 0.5
        want = torch.einsum("hi,hil,lhe->he", coef, s.softmax(-1), v)
        assert rel_err(got[b], want) <= TOL[torch.bfloat16], (b, L)


def test_fp8_placement_independence_bitwise():
    N, hs, dv, P = 2, 64, 128, 64
    q, coef, kb, vb, sc = _inputs(N, hs, dv)
    qd, cd = q.to(DEV, torch.bfloat16), coef.to(DEV)
    lengths = (1, 257, 600)
    outs = []
    for shuffle, seed in ((False, 0), (True, 1), (True, 2)):
        k_pool, v_pool, scales, table = _paginate(kb, vb, sc, lengths, P, CAP, seed=seed, shuffle=shuffle)
        outs.append(ops.diff_attention_decode_paged_fp8(qd, k_pool, v_pool, scales, cd, table, _i32(lengths)))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for b in range(B):                                      # alone in the batch, a smaller pool
        k_pool, v_pool, scales, table = _paginate(kb[b:b + 1], vb[b:b + 1], sc[b:b + 1], lengths[b:b + 1], P, CAP,
                                                  seed=40 + b, spare=1)
        alone = ops.diff_attention_decode_paged_fp8(qd[b:b + 1], k_pool, v_pool, scales, cd, table, _i32(lengths[b:b + 1]))
        assert torch.equal(outs[0][b:b + 1], alone), b


# ------------------------------------------------------------ write kernel ---
def _element_bound(x, scale):
    """2^-4 |x| + 2^-10 scale, plus one fp32 ulp of x / scale (|x / scale| <= 448 < 2^9, so an
    ulp is at most 2^-15) in units of the scale."""
    return x.abs() * 2.0 ** -4 + scale[..., None] * (2.0 ** -10 + 2.0 ** -15)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_kv_quant_rows(dtype, N, hs, dv):
    Bq, Tn, Hq, P, n_pages = 2, 3, 2, 32, 4
    nq = Hq * N * hs
    W = nq + Hq * dv
    g = torch.Generator().manual_seed(17 * N + hs)
    # strided sources: K a temporary of its own, V a slice of a wider packed tensor
    k_new = (torch.randn(Bq, Tn, Hq, N, hs, generator=g) * torch.logspace(-2, 1, Tn)[None, :, None, None, None]).to(DEV, dtype)
    wide = torch.randn(Bq, Tn, 2 * nq + Hq * dv, generator=g).to(DEV, dtype)
    v_new = wide[..., 2 * nq:].unflatten(-1, (Hq, dv))
    k_new[0, 1, 1, 0] = 0                                           # a zero K_i row
    v_new[1, 0, 0] = 0                                              # a zero V row
    pool = torch.full((n_pages + 1, P, W), 0xA5, dtype=torch.uint8, device=DEV)
    scales = torch.full((n_pages + 1, P, Hq, N + 1), -7.0, device=DEV)
    k_pool, v_pool = pool[..., :nq].unflatten(-1, (Hq, N, hs)), pool[..., nq:].unflatten(-1, (Hq, dv))
    last = (n_pages + 1) * P - 1                                    # the last valid index: the spare page's last row
    slots = [3 * P + 5, 0, n_pages * P - 1, 1 * P + 31, last, 2 * P]          # row (1, 1) is the padding row
    args = (k_new, v_new, k_pool, v_pool, scales, _i32(slots))
    if hs % 16:
        with pytest.raises(RuntimeError, match="code -2"):          # DTA_ERR_UNSUPPORTED, nothing written
            ops.kv_quant_rows(*args)
        assert (pool == 0xA5).all() and (scales == -7.0).all()
        return
    snap_pool, snap_scales = pool.clone(), scales.clone()
    ops.kv_quant_rows(*args)
    torch.cuda.synchronize()
    rows = pool.view(-1, W)[slots]                                  # (6, W)
    got_k = rows[:, :nq].view(Bq, Tn, Hq, N, hs)
    got_v = rows[:, nq:].view(Bq, Tn, Hq, dv)
    got_s = scales.view(-1, Hq, N + 1)[slots].view(Bq, Tn, Hq, N + 1)
    for name, x, byte, sc in (("K", k_new.float(), got_k, got_s[..., :N]), ("V", v_new.float(), got_v, got_s[..., N])):
        amax = x.abs().amax(-1)
        assert ((sc - amax / 448.0).abs() <= 1e-6 * amax / 448.0).all(), (name, "scale")
        deq = byte.contiguous().view(torch.float8_e4m3fn).float()
        assert torch.isfinite(deq).all(), name
        err = (deq * sc[..., None] - x).abs()
        bound = _element_bound(x, sc)
        print(f"kv_quant_rows {dtype} N={N} hs={hs} {name}: max err/bound {(err / bound.clamp_min(1e-30)).max().item():.3f}")
        assert (err <= bound).all(), (name, "element bound")
        top = x.abs().argmax(-1, keepdim=True)
        live = amax > 0
        assert (deq.gather(-1, top)[live].abs() == 448.0).all(), (name, "the amax element is +-448")
        assert torch.equal(deq.gather(-1, top).sign()[live], x.gather(-1, top).sign()[live]), name
        assert (sc[~live] == 0).all() and (byte[~live] == 0).all(), (name, "a zero row: scale 0, bytes 0")
    assert not (k_new[0, 1, 1, 0] != 0).any() and got_s[0, 1, 1, 0] == 0 and got_s[1, 0, 0, N] == 0
    # nothing but the named rows changed
    keep = torch.ones((n_pages + 1) * P, dtype=torch.bool, device=DEV)
    keep[slots] = False
    assert torch.equal(pool.view(-1, W)[keep], snap_pool.view(-1, W)[keep])
    assert torch.equal(scales.view(-1, Hq, N + 1)[keep], snap_scales.view(-1, Hq, N + 1)[keep])


# ------------------------------------------------------------- model level ---
BS, P = PG.BS, PG.P


def _bound_rows(x, scale):
    return x.abs() * 2.0 ** -4 + scale * (2.0 ** -10 + 2.0 ** -15)


def _cached_rows(model, cache, seq, layer):
    """(k (L, H, N, hs), v (L, H, dv), scales (L, H, N + 1) or None) of one sequence in one layer."""
    _, Hm, N, hs, dv, _ = kv_cache._spec(model.blocks[layer - 1])
    nq = Hm * N * hs
    L = cache.host_lengths[seq]
    pool = cache.pool[layer][:cache.num_pages]
    k_pool, v_pool = pool[..., :nq].unflatten(-1, (Hm, N, hs)), pool[..., nq:].unflatten(-1, (Hm, dv))
    if cache.kv_dtype is None:
        pages = torch.tensor(cache.pages[seq], device=DEV)
        return k_pool[pages].flatten(0, 1)[:L].float(), v_pool[pages].flatten(0, 1)[:L].float(), None
    s_pool = cache.scale_pool[layer][:cache.num_pages].unflatten(-1, (Hm, N + 1))
    k, v = ops.kv_dequant_reference(k_pool, v_pool, s_pool, cache.pages[seq], L)
    pages = torch.tensor(cache.pages[seq], device=DEV)
    return k, v, s_pool[pages].flatten(0, 1)[:L]


def _check_rows(model, cache, twin, pairs, layers, tag):
    for layer in layers:
        for q8, qt in pairs:
            k8, v8, sc = _cached_rows(model, cache, q8, layer)
            kt, vt, _ = _cached_rows(model, twin, qt, layer)
            N = kt.shape[2]
            assert k8.shape == kt.shape and v8.shape == vt.shape
            assert ((k8 - kt).abs() <= _bound_rows(kt, sc[..., :N, None])).all(), (tag, layer, q8, "K")
            assert ((v8 - vt).abs() <= _bound_rows(vt, sc[..., N, None])).all(), (tag, layer, q8, "V")
            # the scales are those of the twin's rows: a head, branch or index mix-up moves them
            assert torch.allclose(sc[..., :N], kt.abs().amax(-1) / 448.0, rtol=1e-6, atol=0), (tag, layer, q8)
            assert torch.allclose(sc[..., N], vt.abs().amax(-1) / 448.0, rtol=1e-6, atol=0), (tag, layer, q8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_cached_rows_match_an_unquantised_twin(which, dtype):
    model = PG._model(which).to(dtype)
    prompts = PG._prompts(5, [40, 100, 7])
    cache, twin = kv_cache.PagedKVCache(12, P, kv_dtype=FP8), kv_cache.PagedKVCache(12, P)
    with torch.no_grad():
        ids, got = kv_cache.prefill_paged(model, prompts, cache)
        idt, want = kv_cache.prefill_paged(model, prompts, twin)
        assert torch.equal(got, want)              # the prefill's attention runs on unquantised activations in both
        assert cache.pool[1].dtype == torch.uint8 and cache.scale_pool[1].dtype == torch.float32
        _check_rows(model, cache, twin, list(zip(ids, idt)), range(1, len(model.blocks) + 1), (which, "prefill"))
        g = torch.Generator().manual_seed(6)
        for _ in range(2):
            tok = torch.randint(0, 97, (3, 1), generator=g).to(DEV)
            out = kv_cache.decode_paged(model, ids, tok, cache)
            kv_cache.decode_paged(model, idt, tok, twin)
            assert out.shape == (3, 97) and torch.isfinite(out.float()).all()
        assert cache.sync() == dict(zip(ids, [42, 102, 9]))
        _check_rows(model, cache, twin, list(zip(ids, idt)), [1], (which, "decode"))      # layer 1 sees embeddings only


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_fp8_continuous_batching_bitwise(which):
    """Release a sequence, prefill another into its pages: the survivors' logits equal those
    of a cache in which the release never happened (stale bytes and scales in reused pages
    do not leak)."""
    model = PG._model(which)
    pa, pb, pc = PG._prompts(5, [40, 100, 70])
    cache, calm = kv_cache.PagedKVCache(12, P, kv_dtype=FP8), kv_cache.PagedKVCache(12, P, kv_dtype=FP8)
    g = torch.Generator().manual_seed(6)
    toks = [torch.randint(0, 97, (2, 1), generator=g).to(DEV) for _ in range(5)]
    with torch.no_grad():
        (a, b), _ = kv_cache.prefill_paged(model, [pa, pb], cache)
        (a2, b2), _ = kv_cache.prefill_paged(model, [pa, pb], calm)  # the same steps (same GEMM shapes), no release
        for t in toks[:2]:
            kv_cache.decode_paged(model, [a, b], t, cache)
            kv_cache.decode_paged(model, [a2, b2], t, calm)
        a_pages = list(cache.pages[a])
        cache.release(a)
        (c,), got_c = kv_cache.prefill_paged(model, [pc], cache)
        (c2,), want_c = kv_cache.prefill_paged(model, [pc], calm)
        assert set(a_pages) <= set(cache.pages[c])                  # A's pages, reused
        assert torch.equal(got_c, want_c)
        for t in toks[2:]:
            got = kv_cache.decode_paged(model, [c, b], t, cache)
            want = kv_cache.decode_paged(model, [c2, b2], t, calm)
            assert torch.isfinite(got).all() and torch.equal(got, want), which
        assert cache.pages_in_use() == 7 and calm.pages_in_use() == 9


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_fp8_fork_copies_scale_pages_on_write(which):
    model = PG._model(which)
    (prompt,) = PG._prompts(15, [70])                               # one full page of 64 and 6 rows
    cache, twin = kv_cache.PagedKVCache(6, 64, kv_dtype=FP8), kv_cache.PagedKVCache(6, 64, kv_dtype=FP8)
    g = torch.Generator().manual_seed(16)
    t0, t1, t2 = (torch.randint(0, 97, (1, 1), generator=g).to(DEV) for _ in range(3))
    with torch.no_grad():
        (a,), _ = kv_cache.prefill_paged(model, [prompt], cache)
        (never,), _ = kv_cache.prefill_paged(model, [prompt], twin)
        full_page = cache.pages[a][0]
        child = cache.fork(a)
        assert cache.pages_in_use() == 2
        both = kv_cache.decode_paged(model, [a, child], torch.cat([t0, t0]), cache)
        assert torch.equal(both[0], both[1])                        # same next token: same logits, bitwise
        kv_cache.decode_paged(model, [never], t0, twin)
        kv_cache.decode_paged(model, [a], t1, cache)               # the parent advances alone ...
        got = kv_cache.decode_paged(model, [child], t2, cache)      # ... and the child does not see it
        want = kv_cache.decode_paged(model, [never], t2, twin)
        assert torch.equal(got, want), which
    assert [cache.pages[q][0] for q in (a, child)] == [full_page] * 2 and cache.refcount[full_page] == 2
    assert cache.pages[a][1] != cache.pages[child][1] and cache.pages_in_use() == 1 + 2


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_fp8_append_equals_one_at_a_time_decode_bitwise(which):
    model = PG._model(which)
    prompts = PG._prompts(8, [30, 17, 60])
    new = torch.randint(0, 97, (3, 5), generator=torch.Generator().manual_seed(9)).to(DEV)
    cache, step = kv_cache.PagedKVCache(12, P, kv_dtype=FP8), kv_cache.PagedKVCache(12, P, kv_dtype=FP8)
    with torch.no_grad():
        ids, _ = kv_cache.prefill_paged(model, prompts, cache)
        ids2, _ = kv_cache.prefill_paged(model, prompts, step)
        rows = kv_cache.append_paged(model, ids, new, [5, 5, 5], cache, all_rows=True)     # 30 -> 35, 60 -> 65 cross a page
        assert rows.shape == (3, 5, 97)
        for r in range(5):
            want = kv_cache.decode_paged(model, ids2, new[:, r:r + 1], step)
            assert torch.equal(rows[:, r], want), (which, r)
        for layer in cache.pool:
            for q, q2 in zip(ids, ids2):
                ka, va, sa = _cached_rows(model, cache, q, layer)
                kb_, vb_, sb_ = _cached_rows(model, step, q2, layer)
                assert torch.equal(ka, kb_) and torch.equal(va, vb_) and torch.equal(sa, sb_)


def test_generate_paged_fp8():
    model = PG._model("diff")
    prompts = PG._prompts(9, [5, 17, 40])
    seen = {}
    real = kv_cache.PagedKVCache

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen[self.kv_dtype] = self

    kv_cache.PagedKVCache = Spy
    try:
        torch.manual_seed(123)
        plain = kv_cache.generate_paged(model, prompts, 6, page_size=P)
        torch.manual_seed(123)
        got = kv_cache.generate_paged(model, prompts, 6, page_size=P, kv_dtype=FP8)
    finally:
        kv_cache.PagedKVCache = real
    assert len(got) == 3
    for b in range(3):
        assert got[b].shape == plain[b].shape == (prompts[b].shape[0] + 6,)
        assert torch.equal(got[b][:prompts[b].shape[0]], prompts[b])
    c8, cp = seen[FP8], seen[None]
    assert c8.pages_in_use() == cp.pages_in_use() and c8.num_pages == cp.num_pages
    assert c8.pool[1].dtype == torch.uint8 and cp.pool[1].dtype == torch.float32
    # the path is in use: the byte pool is not the plain pool's bytes, and it holds 0.523x-like bytes
    assert c8.pool[1].shape == cp.pool[1].shape and c8.cache_bytes() < cp.cache_bytes()
    assert not torch.equal(c8.pool[1].view(-1)[:4096], cp.pool[1].view(torch.uint8).view(-1)[:4096])
    with torch.no_grad():
        ids = list(c8.slot)
        logits = kv_cache.decode_paged(model, ids, torch.zeros(len(ids), 1, dtype=torch.long, device=DEV), c8)
    assert logits.shape == (3, 97) and torch.isfinite(logits).all()
    with pytest.raises(ValueError):
        kv_cache.generate_paged(model, prompts, 6, kv_dtype="e5m2")
    with pytest.raises(RuntimeError):                               # head size 40: no quantising write, and no fallback
        torch.manual_seed(4)
        m40 = PG.C.StandardTransformer(97, 160, 4, 2, BS, 0.0).to(DEV).eval()
        kv_cache.generate_paged(m40, prompts, 2, kv_dtype=FP8)
