"""GPU parity of the paged KV cache (``dta_attn_decode_paged``, ``dta_attn_extend_paged``):
cache rows reached through a per-sequence block table into a shared pool of pages.

* ``ops.diff_attention_decode_paged`` / ``ops.diff_attention_extend_paged`` against the
  oracle's ``diff_core`` in fp64 (the references of tests/test_gpu_ragged.py, computed once
  and shared), per sequence over its own valid rows, on a pool larger than needed whose
  pages are assigned by a fixed random permutation, with every unowned page and every row
  past a length NaN and the unused table entries -1.
* Bitwise equality with the ragged ops on the gathered contiguous cache at the same
  t_cap (the ordering contract): at a chunk boundary (256 / 257), a page boundary inside
  a chunk, a partial last page, an empty sequence, the single-pass kernel and the
  512-key chunk plan; bitwise independence of a sequence from its batch and from where
  its pages lie.
* The argument contract of the two ops (valid page ids only: the clamp of a bad id is
  checked by reading the kernels, not by feeding one to the device).
* Model level, fp32 at 1e-4 against the model's own full forward of each sequence
  alone: continuous batching on a 12-page pool (release, prefill into the live cache,
  out of pages), ``append_paged`` across a page boundary, ``truncate``, the head-size-40
  fallback, ``fork`` with copy on write, ``generate_paged`` token for token against
  ``generate_ragged``, and shared prompt pages with ``n_samples``.
Tolerances as tests/test_gpu_ragged.py: fp32 max|a-b|/max|b| <= 1e-4, bf16 / f16 <= 2e-2.
"""
import pytest
import torch

import test_gpu_ragged as R
from conftest import rel_err

from differential_transformer_replication_amd import ops, kv_cache
from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import Ndiff_transformer as ND
from differential_transformer_replication_amd import control as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = R.TOL
DTYPES = R.DTYPES
B, H = R.B, R.H
DEC_LENGTHS = R.DEC_LENGTHS + [(0, 5, 600)]
NAN = float("nan")


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _round_up(n, P):
    return -(-n // P) * P


def _paginate(k, v, valid, P, cap, seed, spare=5):
    """Cut the contiguous caches k (B, T, H, N, hs) / v (B, T, H, dv) (device tensors, rows
    valid[b] .. NaN-filled here) into pages of P rows up to ``cap`` rows per sequence and
    scatter them over a packed pool (n_pages, P, [K | V]) by a fixed random permutation.
    Returns (k_pool, v_pool, table, k_cap, v_cap): the strided pool views, the int32 block
    table (unused entries -1; every unowned page and every row past valid[b] is NaN) and
    the contiguous caches padded to ``cap`` rows, poisoned the same way."""
    Bn, T, Hn, N, hs = k.shape
    dv = v.shape[-1]
    nq = Hn * N * hs
    max_pages = cap // P
    cache = torch.full((Bn, cap, nq + Hn * dv), NAN, device=DEV, dtype=k.dtype)
    for b, L in enumerate(valid):
        cache[b, :L, :nq] = k[b, :L].flatten(1)
        cache[b, :L, nq:] = v[b, :L].flatten(1)
    n_pages = Bn * max_pages + spare
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[:Bn * max_pages].view(Bn, max_pages)
    pool = torch.full((n_pages, P, nq + Hn * dv), NAN, device=DEV, dtype=k.dtype)
    table = torch.full((Bn, max_pages), -1, dtype=torch.int32)
    for b, L in enumerate(valid):
        for p in range(-(-L // P)):
            table[b, p] = perm[b, p]
            pool[perm[b, p]] = cache[b, p * P:(p + 1) * P]
    k_pool = pool[..., :nq].unflatten(-1, (Hn, N, hs))
    v_pool = pool[..., nq:].unflatten(-1, (Hn, dv))
    k_cap = cache[..., :nq].unflatten(-1, (Hn, N, hs))
    v_cap = cache[..., nq:].unflatten(-1, (Hn, dv))
    return k_pool, v_pool, table.to(DEV), k_cap, v_cap


# ------------------------------------------------------------------ decode ---
@pytest.mark.parametrize("P", [32, 64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", R.DEC_SHAPES)
def test_decode_paged_matches_oracle_and_ragged_bitwise(dtype, N, hs, dv, P):
    q, k, v, coef = R._dec_inputs(N, hs, dv)
    qd, kd, vd, cd = q.to(DEV, dtype), k.to(DEV, dtype), v.to(DEV, dtype), coef.to(DEV)
    cap = _round_up(R.DEC_CAP, P)
    for lengths in DEC_LENGTHS:
        k_pool, v_pool, table, k_cap, v_cap = _paginate(kd, vd, lengths, P, cap, seed=P + sum(lengths))
        got = ops.diff_attention_decode_paged(qd, k_pool, v_pool, cd, table, _i32(lengths))
        assert got.shape == (B, H * dv) and got.dtype == dtype
        same = ops.diff_attention_decode_ragged(qd, k_cap, v_cap, cd, _i32(lengths))
        assert torch.equal(got, same), (dtype, N, hs, P, lengths, "paged != ragged on the gathered cache")
        tight = ops.diff_attention_decode_paged(qd, k_pool, v_pool, cd, table, _i32(lengths), max(max(lengths), 1))
        assert torch.equal(tight, got), (dtype, N, hs, P, lengths, "max_length moved the result")
        got = got.view(B, H, dv).float().cpu()
        assert torch.isfinite(got).all(), (dtype, N, hs, P, lengths)
        want = R._dec_want(N, hs, dv, lengths)
        for b, L in enumerate(lengths):
            if L == 0:
                assert (got[b] == 0).all(), (dtype, N, hs, P, "an empty sequence writes zeros")
            else:
                err = rel_err(got[b], want[b])
                print(f"decode_paged {dtype} N={N} hs={hs} dv={dv} P={P} len={L}: rel_err {err:.3e}")
                assert err <= TOL[dtype], (dtype, N, hs, dv, P, lengths, b)


def test_decode_paged_wide_chunk_plan_bitwise():
    """ceil(t_cap / 256) * H * B >= 8192: the 512-key chunk plan (8 pages of 64 per chunk).
    Bitwise only, inputs made on the device."""
    Bw, Hw, N, hs, dv, P, cap = 8, 16, 2, 32, 64, 64, 16384
    assert -(-cap // 256) * Hw * Bw >= 8192
    g = torch.Generator(device=DEV).manual_seed(5)
    nq = Hw * N * hs
    cache = torch.randn(Bw, cap, nq + Hw * dv, device=DEV, dtype=torch.bfloat16, generator=g)
    q = torch.randn(Bw, Hw, N, hs, device=DEV, dtype=torch.bfloat16, generator=g)
    coef = torch.tensor([[1.0, -0.6]] * Hw, device=DEV)
    lengths = _i32([1, 511, 512, 513, cap, 9000, 777, 12345])
    n_pages = Bw * cap // P
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(6)).to(DEV)
    pool = torch.empty(n_pages, P, nq + Hw * dv, device=DEV, dtype=torch.bfloat16)
    pool[perm] = cache.view(n_pages, P, -1)
    table = perm.view(Bw, cap // P).to(torch.int32)
    got = ops.diff_attention_decode_paged(q, pool[..., :nq].unflatten(-1, (Hw, N, hs)),
                                          pool[..., nq:].unflatten(-1, (Hw, dv)), coef, table, lengths)
    want = ops.diff_attention_decode_ragged(q, cache[..., :nq].unflatten(-1, (Hw, N, hs)),
                                            cache[..., nq:].unflatten(-1, (Hw, dv)), coef, lengths)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------ extend ---
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", R.EXT_SHAPES)
def test_extend_paged_matches_oracle_and_ragged_bitwise(dtype, N, hs, dv, P):
    assert ops.extend_supported(dtype, hs, N, dv)          # a missing plan cannot hide behind a fallback
    for pos, counts, Tq, cap0 in R.EXT_CASES:
        q, k, v, coef, want = R._ext_case(N, hs, dv, pos, counts, Tq, cap0)
        qd, kd, vd, cd = q.to(DEV, dtype), k.to(DEV, dtype), v.to(DEV, dtype), coef.to(DEV)
        cap = _round_up(cap0, P)
        n = [Tq] * B if counts is None else list(counts)
        valid = [pos[b] + n[b] for b in range(B)]
        k_pool, v_pool, table, k_cap, v_cap = _paginate(kd, vd, valid, P, cap, seed=P + Tq)
        cnt = None if counts is None else _i32(counts)
        got = ops.diff_attention_extend_paged(qd, k_pool, v_pool, cd, table, _i32(pos), cnt)
        assert got.shape == (B, Tq, H * dv) and got.dtype == dtype
        same = ops.diff_attention_extend_ragged(qd, k_cap, v_cap, cd, _i32(pos), cnt)
        assert torch.equal(got, same), (dtype, N, hs, P, pos, counts, "paged != ragged on the gathered cache")
        got = got.view(B, Tq, H, dv).float().cpu()
        assert torch.isfinite(got).all(), (dtype, N, hs, P, pos, counts)
        for b in range(B):
            assert (got[b, n[b]:] == 0).all(), (dtype, N, hs, P, b, "padding rows are zeros")
            if n[b]:
                err = rel_err(got[b, :n[b]], want[b, :n[b]])
                print(f"extend_paged {dtype} N={N} hs={hs} dv={dv} P={P} pos={pos[b]} count={n[b]}: rel_err {err:.3e}")
                assert err <= TOL[dtype], (dtype, N, hs, dv, P, pos, counts, b)


# ------------------------------------------------------------ independence ---
def test_sequences_are_independent_of_batch_and_placement_bitwise():
    N, hs, dv, P = 2, 64, 128, 64
    q, k, v, coef = (t.to(DEV) for t in R._dec_inputs(N, hs, dv))
    cap = _round_up(R.DEC_CAP, P)
    lengths = (1, 257, 600)
    k_pool, v_pool, table, _, _ = _paginate(k, v, lengths, P, cap, seed=1)
    got = ops.diff_attention_decode_paged(q, k_pool, v_pool, coef, table, _i32(lengths))
    for b in range(B):                                      # alone, its pages somewhere else, a smaller pool
        kp, vp, tb, _, _ = _paginate(k[b:b + 1], v[b:b + 1], lengths[b:b + 1], P, cap, seed=40 + b, spare=1)
        alone = ops.diff_attention_decode_paged(q[b:b + 1], kp, vp, coef, tb, _i32(lengths[b:b + 1]))
        assert torch.equal(got[b:b + 1], alone), b
    k_pool, v_pool, table, _, _ = _paginate(k, v, (600, 257, 3), P, cap, seed=2)
    moved = ops.diff_attention_decode_paged(q, k_pool, v_pool, coef, table, _i32((600, 257, 3)))
    assert torch.equal(moved[1], got[1])
    assert not torch.equal(moved[0], got[0])

    pos, counts, Tq, cap0 = R.EXT_CASES[0]
    q, k, v, coef, _ = R._ext_case(N, hs, dv, pos, counts, Tq, cap0)
    q, k, v, coef = (t.to(DEV) for t in (q, k, v, coef))
    cap = _round_up(cap0, P)
    valid = [p + c for p, c in zip(pos, counts)]
    k_pool, v_pool, table, _, _ = _paginate(k, v, valid, P, cap, seed=3)
    got = ops.diff_attention_extend_paged(q, k_pool, v_pool, coef, table, _i32(pos), _i32(counts))
    for b in range(B):
        kp, vp, tb, _, _ = _paginate(k[b:b + 1], v[b:b + 1], valid[b:b + 1], P, cap, seed=50 + b, spare=1)
        alone = ops.diff_attention_extend_paged(q[b:b + 1], kp, vp, coef, tb, _i32(pos[b:b + 1]), _i32(counts[b:b + 1]))
        assert torch.equal(got[b:b + 1], alone), b


# ---------------------------------------------------------------- contract ---
def test_paged_contract():
    q = torch.zeros(2, 4, 1, 2, 64, device=DEV)
    k = torch.zeros(6, 32, 1, 2, 64, device=DEV)
    v = torch.zeros(6, 32, 1, 128, device=DEV)
    coef = torch.ones(1, 2, device=DEV)
    good = _i32([1, 2])
    table = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=DEV)
    out = ops.diff_attention_decode_paged(q[:, 0], k, v, coef, table, good)
    assert out.shape == (2, 128) and (out == 0).all()
    out = ops.diff_attention_extend_paged(q, k, v, coef, table, good)
    assert out.shape == (2, 4, 128) and (out == 0).all()
    bad_tables = [table.long(), table.float(),                           # dtype
                  table[0], table[:1], table.view(2, 3, 1),              # shape
                  table.cpu(),                                           # device
                  torch.stack([table, table], dim=2)[..., 0],            # not contiguous
                  None]
    for t in bad_tables:
        with pytest.raises(RuntimeError):
            ops.diff_attention_decode_paged(q[:, 0], k, v, coef, t, good)
        with pytest.raises(RuntimeError):
            ops.diff_attention_extend_paged(q, k, v, coef, t, good)
    for P in (48, 16, 512):                                              # page size
        kp = torch.zeros(6, P, 1, 2, 64, device=DEV)
        vp = torch.zeros(6, P, 1, 128, device=DEV)
        with pytest.raises(RuntimeError):
            ops.diff_attention_decode_paged(q[:, 0], kp, vp, coef, table, good)
        with pytest.raises(RuntimeError):
            ops.diff_attention_extend_paged(q, kp, vp, coef, table, good)
    for kk, vv in ((k.bfloat16(), v), (k, v.half()), (k[:5], v), (k, v[:, :16]), (k[0], v[0])):   # dtypes / shapes
        with pytest.raises(RuntimeError):
            ops.diff_attention_decode_paged(q[:, 0], kk, vv, coef, table, good)
        with pytest.raises(RuntimeError):
            ops.diff_attention_extend_paged(q, kk, vv, coef, table, good)
    for t in (torch.tensor([1, 2], device=DEV), _i32([1, 2, 3]), torch.tensor([1, 2], dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            ops.diff_attention_decode_paged(q[:, 0], k, v, coef, table, t)
        with pytest.raises(RuntimeError):
            ops.diff_attention_extend_paged(q, k, v, coef, table, t)
        with pytest.raises(RuntimeError):
            ops.diff_attention_extend_paged(q, k, v, coef, table, good, t)
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_paged(q[:, 0], k, v, coef, table, good, 97)          # max_length > 3 * 32
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_paged(q[:, 0], k, v, coef, table, good, 0)
    with pytest.raises(RuntimeError):                                                  # Tq > max_pages * P
        ops.diff_attention_extend_paged(torch.zeros(2, 97, 1, 2, 64, device=DEV), k, v, coef, table, good)
    with pytest.raises(RuntimeError):                                                  # no extend plan at head size 40
        ops.diff_attention_extend_paged(torch.zeros(2, 4, 1, 2, 40, device=DEV), torch.zeros(6, 32, 1, 2, 40, device=DEV),
                                        torch.zeros(6, 32, 1, 80, device=DEV), coef, table, good)
    out = ops.diff_attention_extend_paged(q[:, :0], k, v, coef, table, good)           # Tq = 0
    assert out.shape == (2, 0, 128)


# ------------------------------------------------------------- model level ---
BS, P, POOL = 256, 32, 12


def _models():
    torch.manual_seed(0)
    yield "diff", D.DiffTransformer(vocab_size=97, n_embd=256, n_head=2, n_layer=2, block_size=BS, dropout=0.0)
    torch.manual_seed(1)
    yield "alt3", ND.AlternatingDiffTransformer(97, 256, 2, 2, BS, 0.0, n_terms=3)
    torch.manual_seed(2)
    yield "ctrl", C.StandardTransformer(97, 256, 4, 2, BS, 0.0)        # N = 1, dv = hs = 64, RoPE


def _model(which):
    model = dict(_models())[which].to(DEV).eval()
    for p in model.parameters():          # non-zero lambdas so every branch weight differs
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model


def _prompts(seed, lens):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in lens]


def _full(model, seq):
    """The model's own full forward of one sequence alone: (T, vocab)."""
    return model(seq[None])[0][0]


def _decode_and_check(model, cache, ids, texts, g, steps, tag):
    """Teacher-forced decode steps of the sequences ``ids`` together; ``texts`` (id -> tokens) follows."""
    for step in range(steps):
        tok = torch.randint(0, 97, (len(ids), 1), generator=g).to(DEV)
        got = kv_cache.decode_paged(model, ids, tok, cache)
        for b, q in enumerate(ids):
            texts[q] = torch.cat([texts[q], tok[b]])
            assert rel_err(got[b], _full(model, texts[q])[-1]) <= 1e-4, (tag, step, q)


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_continuous_batching(which):
    """Four sequences pass through a 12-page pool; a dense cache for them would hold 4 * 8 pages."""
    model = _model(which)
    pa, pb, pc = _prompts(5, [40, 100, 70])
    g = torch.Generator().manual_seed(6)
    cache = kv_cache.PagedKVCache(POOL, P)
    with torch.no_grad():
        (a, b), got = kv_cache.prefill_paged(model, [pa, pb], cache)
        assert got.shape == (2, 97) and cache.pages_in_use() == 6
        texts = {a: pa, b: pb}
        for i, q in enumerate((a, b)):
            assert rel_err(got[i], _full(model, texts[q])[-1]) <= 1e-4, (which, "prefill", q)
        _decode_and_check(model, cache, [a, b], texts, g, 3, (which, "A+B"))
        a_pages = list(cache.pages[a])
        cache.release(a)
        (c,), got = kv_cache.prefill_paged(model, [pc], cache)              # joins the live cache
        texts[c] = pc
        assert set(a_pages) <= set(cache.pages[c]) and len(cache.pages[c]) == 3      # A's pages, reused
        assert rel_err(got[0], _full(model, pc)[-1]) <= 1e-4, (which, "prefill C")
        _decode_and_check(model, cache, [b, c], texts, g, 3, (which, "B+C"))
        assert cache.pages_in_use() == 7 and cache.sync() == {b: 106, c: 73}
        assert cache.lengths[[cache.slot[b], cache.slot[c]]].tolist() == [106, 73]
        with pytest.raises(kv_cache.OutOfPages):                                     # 7 pages, 5 free
            kv_cache.prefill_paged(model, _prompts(7, [200]), cache)
        assert cache.pages_in_use() == 7
        _decode_and_check(model, cache, [c, b], texts, g, 2, (which, "after OutOfPages"))


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_append_truncate_decode(which):
    model = _model(which)
    lens = [30, 17, 60]
    prompts = _prompts(8, lens)
    g = torch.Generator().manual_seed(9)
    cache = kv_cache.PagedKVCache(POOL, P)
    with torch.no_grad():
        ids, _ = kv_cache.prefill_paged(model, prompts, cache)
        assert cache.pages_in_use() == 4
        new = torch.randint(0, 97, (3, 5), generator=g).to(DEV)
        counts = [3, 0, 5]                                                   # 30 -> 33 and 60 -> 65 cross a page boundary
        rows = kv_cache.append_paged(model, ids, new, counts, cache, all_rows=True)
        assert rows.shape == (3, 5, 97) and cache.pages_in_use() == 6
        assert cache.lengths[[cache.slot[q] for q in ids]].tolist() == [33, 17, 65]
        texts = {q: torch.cat([p, new[i, :counts[i]]]) for i, (q, p) in enumerate(zip(ids, prompts))}
        for i in (0, 2):
            want = _full(model, texts[ids[i]])[-counts[i]:]
            assert rel_err(rows[i, :counts[i]], want) <= 1e-4, (which, "append", i)
        last = kv_cache.append_paged(model, [ids[1], ids[2]], new[1:, :2], [2, 1], cache)     # the last real rows
        texts[ids[1]] = torch.cat([texts[ids[1]], new[1, :2]])
        texts[ids[2]] = torch.cat([texts[ids[2]], new[2, :1]])
        for i, q in enumerate((ids[1], ids[2])):
            assert rel_err(last[i], _full(model, texts[q])[-1]) <= 1e-4, (which, "append last", q)
        # roll back: sequence 0 to 31 rows (its second page goes back), sequence 2 to 64
        cache.truncate(ids[0], 31)
        cache.truncate(ids[2], 64)
        assert cache.pages_in_use() == 4
        texts[ids[0]], texts[ids[2]] = texts[ids[0]][:31], texts[ids[2]][:64]
        _decode_and_check(model, cache, ids, texts, g, 2, (which, "after truncate"))
        assert cache.pages_in_use() == 6 and cache.sync() == {ids[0]: 33, ids[1]: 21, ids[2]: 66}


def test_append_paged_fallback_head_size_40():
    """hs = 40 has no extend plan: the paged multi-row step runs one paged decode per row."""
    torch.manual_seed(4)
    model = C.StandardTransformer(97, 160, 4, 2, BS, 0.0).to(DEV).eval()      # hs = dv = 40, N = 1
    assert not ops.extend_supported(torch.float32, 40, 1, 40)
    lens = [30, 17, 60]
    prompts = _prompts(13, lens)
    new = torch.randint(0, 97, (3, 5), generator=torch.Generator().manual_seed(14)).to(DEV)
    counts = [3, 0, 5]
    cache = kv_cache.PagedKVCache(POOL, P)
    with torch.no_grad():
        ids, _ = kv_cache.prefill_paged(model, prompts, cache)
        rows = kv_cache.append_paged(model, ids, new, counts, cache, all_rows=True)
        for i in (0, 2):
            seq = torch.cat([prompts[i], new[i, :counts[i]]])
            assert rel_err(rows[i, :counts[i]], _full(model, seq)[-counts[i]:]) <= 1e-4, i


def test_append_paged_fallback_equals_append_ragged_bitwise():
    """The per-row fallback (hs = 40) of the paged multi-row step gives the ragged one's real rows, bit for bit."""
    torch.manual_seed(4)
    model = C.StandardTransformer(97, 160, 4, 2, 64, 0.0).to(DEV).eval()      # hs = dv = 40, N = 1, fp32
    assert not ops.extend_supported(torch.float32, 40, 1, 40)
    prompts = _prompts(13, [5, 17, 40])
    new = torch.randint(0, 97, (3, 4), generator=torch.Generator().manual_seed(14)).to(DEV)
    counts = [4, 0, 2]
    ragged, paged = kv_cache.RaggedKVCache(), kv_cache.PagedKVCache(POOL, 32)
    with torch.no_grad():
        kv_cache.prefill_ragged(model, prompts, ragged)
        ids, _ = kv_cache.prefill_paged(model, prompts, paged)
        want = kv_cache.append_ragged(model, new, counts, ragged, all_rows=True)
        got = kv_cache.append_paged(model, ids, new, counts, paged, all_rows=True)
    assert got.shape == want.shape == (3, 4, 97)
    for b, c in enumerate(counts):
        assert torch.equal(got[b, :c], want[b, :c]), b
    assert [paged.sync()[q] for q in ids] == ragged.sync() == [9, 17, 42]
    assert paged.lengths[[paged.slot[q] for q in ids]].tolist() == ragged.lengths.tolist() == [9, 17, 42]


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_fork_shares_pages_and_copies_on_write(which):
    model = _model(which)
    (prompt,) = _prompts(15, [70])                                          # one full page of 64 and 6 rows
    g = torch.Generator().manual_seed(16)
    cache = kv_cache.PagedKVCache(6, 64)
    with torch.no_grad():
        (a,), _ = kv_cache.prefill_paged(model, [prompt], cache)
        full_page = cache.pages[a][0]
        ids = [a, cache.fork(a), cache.fork(a)]
        assert cache.pages_in_use() == 2
        texts = {q: prompt for q in ids}
        _decode_and_check(model, cache, ids, texts, g, 2, (which, "forks"))        # three different tokens per step
        assert not torch.equal(texts[ids[0]], texts[ids[1]]) and not torch.equal(texts[ids[1]], texts[ids[2]])
    assert [cache.pages[q][0] for q in ids] == [full_page] * 3 and cache.refcount[full_page] == 3
    assert len({cache.pages[q][1] for q in ids}) == 3
    assert cache.pages_in_use() == 1 + 3


def test_generate_paged_equals_generate_ragged():
    """Every kernel is bitwise the ragged one and everything else is the same torch op on
    the same values, so under one seed the sampled tokens are the same (fp32)."""
    model = _model("diff")
    prompts = _prompts(9, [5, 17, 40])
    torch.manual_seed(123)
    want = kv_cache.generate_ragged(model, prompts, 6)
    torch.manual_seed(123)
    got = kv_cache.generate_paged(model, prompts, 6, page_size=P)
    assert len(got) == 3
    for b in range(3):
        assert torch.equal(got[b], want[b]), b
    with pytest.raises(ValueError):
        kv_cache.generate_paged(model, prompts, 217)                       # 40 + 217 > 256


def test_generate_paged_shares_the_prompt_pages():
    model = _model("ctrl")
    prompts = _prompts(10, [70, 40])
    # P = 32, 4 new tokens (3 cached): 70 -> two shared full pages + 3 own; 40 -> one shared + 3 own
    need = (2 + 3) + (1 + 3)
    torch.manual_seed(7)
    out = kv_cache.generate_paged(model, prompts, 4, n_samples=3, num_pages=need, page_size=P)
    assert len(out) == 2 and all(len(o) == 3 for o in out)
    for b, samples in enumerate(out):
        for s in samples:
            assert s.shape == (prompts[b].shape[0] + 4,) and torch.equal(s[:prompts[b].shape[0]], prompts[b])
    torch.manual_seed(7)
    again = kv_cache.generate_paged(model, prompts, 4, n_samples=3, page_size=P)       # the default is that need
    assert all(torch.equal(x, y) for xs, ys in zip(out, again) for x, y in zip(xs, ys))
    with pytest.raises(kv_cache.OutOfPages):                                           # unshared it would take 15
        kv_cache.generate_paged(model, prompts, 4, n_samples=3, num_pages=need - 1, page_size=P)
