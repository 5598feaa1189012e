"""Split-key decode for a step of 2 .. 8 rows (``ops.diff_attention_decode_rows*``).

Every real row is pinned bit for bit to the one-row decode op at lengths = pos + r + 1 on the
same cache (contiguous, paged, fp8 pages), at the smallest shape that has three 256-key chunks:
B 3, H 2, t_cap 768, pos (253, 0, 505) -- sequence 0's rows straddle the first chunk boundary
(its early rows have no partial in chunk 1), sequence 1 starts at an empty cache, sequence 2
straddles the second boundary -- and counts (Tq, min(Tq, 3), Tq).  Then the CPU oracle, padding
and empty sequences, poisoned tails inside guard bands, the 512-key chunk plan, the clamps of
the device values, independence of the batch, and the model-level dispatch behind
``rows_decode=True``."""
import functools

import pytest
import torch

import test_gpu_fp8_cache as F8
import test_gpu_paged as PG
import test_gpu_poison as PZ
import test_gpu_ragged as R
from _poison import poisoned_allocations
from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import kv_cache, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = R.TOL                       # test_decode_ragged_matches_oracle's
DTYPES = R.DTYPES
B, H = R.B, R.H
assert (B, H) == (3, 2)
CAP, P = 768, 64
POS = (253, 0, 505)
SHAPES = [(2, 32, 64), (2, 64, 128), (2, 128, 256), (3, 64, 128), (1, 64, 64)]       # (N, hs, dv)
TQS = [2, 5, 8]
NAN = float("nan")
_i32 = R._i32


def _counts(Tq):
    return (Tq, min(Tq, 3), Tq)


@functools.lru_cache(maxsize=None)
def _inputs(N, hs, dv):
    """Host tensors, made once per shape and shared: q for 8 rows, CAP cache rows, coef, and the
    quantised rows with their scales."""
    g = torch.Generator().manual_seed(17 * N + hs + dv)
    q = torch.randn(B, 8, H, N, hs, generator=g)
    k = torch.randn(B, CAP, H, N, hs, generator=g)
    v = torch.randn(B, CAP, H, dv, generator=g)
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    kb, ks = ops.kv_quant_reference(k)
    vb, vs = ops.kv_quant_reference(v)
    return q, k, v, coef, kb, vb, torch.cat([ks, vs[..., None]], dim=-1)


@functools.lru_cache(maxsize=None)
def _want(N, hs, dv, Tq, fp8_dtype=None):
    """The oracle's rows pos: of the full causal forward over pos + count rows, per sequence
    (fp64; ``fp8_dtype``: fp32 on the dequantised rows with q rounded to that dtype, as
    test_gpu_fp8_cache._want)."""
    q, k, v, coef, kb, vb, sc = _inputs(N, hs, dv)
    dt = torch.float64
    if fp8_dtype is not None:
        dt = torch.float32
        q = q.to(fp8_dtype)
        k = kb.view(torch.float8_e4m3fn).float() * sc[..., :N, None]
        v = vb.view(torch.float8_e4m3fn).float() * sc[..., N, None]
    want = torch.zeros(B, Tq, H, dv, dtype=dt)
    for b, n in enumerate(_counts(Tq)):
        L = POS[b] + n
        for h in range(H):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs, dtype=dt)
                rows[0, POS[b]:] = q[b, :n, h, i].to(dt)
                qs.append(rows)
            o = O.diff_core(qs, [k[b:b + 1, :L, h, i].to(dt) for i in range(N)], v[b:b + 1, :L, h].to(dt),
                            coef[h].to(dt))
            want[b, :n, h] = o[0, POS[b]:]
    return want


def _caches(dtype, N, hs, dv, Tq, pos=POS, counts=None):
    """The three caches of one case, everything at or past pos + count poisoned: the contiguous
    (k, v), the pages (k_pool, v_pool, table) shuffled over a pool, the fp8 pages with scales."""
    q, k, v, coef, kb, vb, sc = _inputs(N, hs, dv)
    counts = _counts(Tq) if counts is None else counts
    valid = [p + n if n else 0 for p, n in zip(pos, counts)]
    kd, vd = k.to(DEV, dtype), v.to(DEV, dtype)
    k_pool, v_pool, table, k_cap, v_cap = PG._paginate(kd, vd, valid, P, CAP, seed=Tq + sum(valid))
    f8 = F8._paginate(kb, vb, sc, valid, P, CAP, seed=Tq + sum(valid) + 1)
    return q[:, :Tq].to(DEV, dtype), coef.to(DEV), (k_cap, v_cap), (k_pool, v_pool, table), f8


def _rows_all(qd, cd, contig, paged, f8, pos, counts):
    return (ops.diff_attention_decode_rows(qd, *contig, cd, pos, counts),
            ops.diff_attention_decode_rows_paged(qd, *paged[:2], cd, paged[2], pos, counts),
            ops.diff_attention_decode_rows_paged_fp8(qd, *f8[:3], cd, f8[3], pos, counts))


def _per_row(qd, cd, contig, paged, f8, r, lengths):
    ln = _i32(lengths)
    return (ops.diff_attention_decode_ragged(qd[:, r], *contig, cd, ln),
            ops.diff_attention_decode_paged(qd[:, r], *paged[:2], cd, paged[2], ln),
            ops.diff_attention_decode_paged_fp8(qd[:, r], *f8[:3], cd, f8[3], ln))


@pytest.mark.parametrize("Tq", TQS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_rows_equal_the_per_row_decode_bitwise_and_match_the_oracle(dtype, N, hs, dv, Tq):
    assert ops.decode_rows_supported(dtype, hs, N, dv, Tq) and ops.decode_rows_supported(dtype, hs, N, dv, Tq, fp8=True)
    counts = _counts(Tq)
    qd, cd, contig, paged, f8 = _caches(dtype, N, hs, dv, Tq)
    got = _rows_all(qd, cd, contig, paged, f8, _i32(POS), _i32(counts))
    names = ("contiguous", "paged", "fp8")
    for g in got:
        assert g.shape == (B, Tq, H * dv) and g.dtype == dtype
        assert torch.isfinite(g.float()).all()
    for r in range(Tq):
        real = [b for b in range(B) if r < counts[b]]
        lengths = [POS[b] + r + 1 if b in real else 0 for b in range(B)]
        for name, g, one in zip(names, got, _per_row(qd, cd, contig, paged, f8, r, lengths)):
            for b in range(B):
                if b in real:
                    assert torch.equal(g[b, r], one[b]), (name, dtype, N, hs, dv, Tq, b, r, "not the one-row decode")
                else:
                    assert (g[b, r] == 0).all(), (name, dtype, N, hs, dv, Tq, b, r, "a padding row is zeros")
    assert torch.equal(got[0], got[1]), "paged != contiguous"
    for name, g, want in ((names[0], got[0], _want(N, hs, dv, Tq)), (names[2], got[2], _want(N, hs, dv, Tq, dtype))):
        g = g.view(B, Tq, H, dv).float().cpu()
        for b, n in enumerate(counts):
            err = rel_err(g[b, :n], want[b, :n])
            print(f"decode_rows {name} {dtype} N={N} hs={hs} dv={dv} Tq={Tq} pos={POS[b]} count={n}: rel_err {err:.3e}")
            assert err <= TOL[dtype], (name, dtype, N, hs, dv, Tq, b)


def test_empty_sequences_and_empty_batches():
    """count_b = 0 leaves zeros whatever its cache holds; B = 0 and H = 0 return without a launch."""
    N, hs, dv, Tq, dtype = 2, 64, 128, 5, torch.bfloat16
    counts = (0, 2, 0)
    qd, cd, contig, paged, f8 = _caches(dtype, N, hs, dv, Tq, counts=counts)       # every row of 0 and 2 is poison
    got = _rows_all(qd, cd, contig, paged, f8, _i32(POS), _i32(counts))
    clean = _caches(dtype, N, hs, dv, Tq, counts=(Tq, 2, Tq))
    ref = _rows_all(*clean, _i32(POS), _i32(counts))
    for g, w in zip(got, ref):
        assert torch.isfinite(g.float()).all()
        assert (g[0] == 0).all() and (g[2] == 0).all() and (g[1, 2:] == 0).all()
        assert torch.equal(g, w), "an empty sequence's cache contents reached the output"
    z = torch.zeros(0, dtype=torch.int32, device=DEV)
    out = ops.diff_attention_decode_rows(qd[:0], contig[0][:0], contig[1][:0], cd, z, z)
    assert out.shape == (0, Tq, H * dv)
    out = ops.diff_attention_decode_rows(qd[:, :, :0], contig[0][:, :, :0], contig[1][:, :, :0], cd[:0], _i32(POS))
    assert out.shape == (B, Tq, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", [(2, 64, 128), (3, 64, 128)])
def test_poisoned_tails_inside_guard_bands(dtype, N, hs, dv):
    """Everything at or past pos + count is NaN (cache rows, unowned pages, their fp8 scales; the
    table entries past the used pages are garbage); outputs and workspace sit in guard bands."""
    Tq = 5
    counts = _counts(Tq)
    qd, cd, contig, paged, f8 = _caches(dtype, N, hs, dv, Tq)
    pos, cnt = _i32(POS), _i32(counts)
    nq = H * N * hs
    table = paged[2].clone()
    table[table < 0] = 10 ** 6                                                   # never read; clamped if it were
    f8_table = f8[3].clone()
    f8_table[f8_table < 0] = -(10 ** 6)
    plain = _rows_all(qd, cd, contig, (paged[0], paged[1], table), (f8[0], f8[1], f8[2], f8_table), pos, cnt)
    with poisoned_allocations() as s:
        cache = s.guarded(contig[0]._base, "cache")
        kc, vc = cache[..., :nq].unflatten(-1, (H, N, hs)), cache[..., nq:].unflatten(-1, (H, dv))
        a = ops.diff_attention_decode_rows(s.guarded(qd, "q"), kc, vc, s.guarded(cd, "coef"), s.guarded(pos, "pos"),
                                           s.guarded(cnt, "counts"))
        s.verify(*PZ.DECODE)
    assert s.names() == ["o", "ws"]
    with poisoned_allocations() as s:
        kp, vp = PZ._repool(s, paged[0], nq, (H, N, hs), (H, dv), "pool")
        b = ops.diff_attention_decode_rows_paged(s.guarded(qd, "q"), kp, vp, s.guarded(cd, "coef"),
                                                 s.guarded(table, "block_table"), s.guarded(pos, "pos"),
                                                 s.guarded(cnt, "counts"))
        s.verify(*PZ.DECODE)
    assert s.names() == ["o", "ws"]
    with poisoned_allocations() as s:
        kp, vp = PZ._repool(s, f8[0], nq, (H, N, hs), (H, dv), "byte_pool")
        c = ops.diff_attention_decode_rows_paged_fp8(s.guarded(qd, "q"), kp, vp, s.guarded(f8[2], "scale_pool"),
                                                     s.guarded(cd, "coef"), s.guarded(f8_table, "block_table"),
                                                     s.guarded(pos, "pos"), s.guarded(cnt, "counts"))
        s.verify(*PZ.DECODE)
    assert s.names() == ["o", "ws"]
    PZ._same((a, b, c), plain, ("o contiguous", "o paged", "o fp8"))
    for g in (a, b, c):
        assert torch.isfinite(g.float()).all()


def test_wide_chunk_plan_bitwise():
    """ceil(t_cap / 256) * H * B >= 8192: the 512-key chunk plan, built as
    test_decode_paged_wide_chunk_plan_bitwise builds it, over a pool of a few pages; rows that
    straddle the 512- and 1024-key boundaries, for the 16-bit and the fp8 pool."""
    Bw, Hw, N, hs, dv, cap, Tq = 8, 16, 2, 32, 64, 32768, 8
    assert -(-cap // 256) * Hw * Bw >= 8192
    pos = [508, 0, 1020, 511, 505, 1017, 3, 512]
    valid = [p + Tq for p in pos]
    g = torch.Generator().manual_seed(9)
    q = torch.randn(Bw, Tq, Hw, N, hs, generator=g).to(DEV, torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * Hw, device=DEV)
    k = torch.randn(3, 1088, Hw, N, hs, generator=g)
    v = torch.randn(3, 1088, Hw, dv, generator=g)
    pick = [b % 3 for b in range(Bw)]
    wide = lambda t: torch.cat([t, torch.full((Bw, cap // P - t.shape[1]), -1, dtype=torch.int32, device=DEV)],
                               dim=1).contiguous()
    k_pool, v_pool, table, _, _ = PG._paginate(k[pick].to(DEV, torch.bfloat16), v[pick].to(DEV, torch.bfloat16), valid, P,
                                               1088, seed=3)
    kb, ks = ops.kv_quant_reference(k)
    vb, vs = ops.kv_quant_reference(v)
    sc = torch.cat([ks, vs[..., None]], dim=-1)
    kq, vq, scales, table8 = F8._paginate(kb[pick], vb[pick], sc[pick], valid, P, 1088, seed=4)
    table, table8 = wide(table), wide(table8)
    got = ops.diff_attention_decode_rows_paged(q, k_pool, v_pool, coef, table, _i32(pos))
    got8 = ops.diff_attention_decode_rows_paged_fp8(q, kq, vq, scales, coef, table8, _i32(pos))
    assert torch.isfinite(got.float()).all() and torch.isfinite(got8.float()).all()
    for r in range(Tq):
        ln = _i32([p + r + 1 for p in pos])
        assert torch.equal(got[:, r], ops.diff_attention_decode_paged(q[:, r], k_pool, v_pool, coef, table, ln)), r
        assert torch.equal(got8[:, r], ops.diff_attention_decode_paged_fp8(q[:, r], kq, vq, scales, coef, table8, ln)), r


def test_device_values_are_clamped():
    """As test_gpu_ragged.test_device_values_are_clamped: only values whose clamped result is
    well defined, on a fully valid cache.  pos -5 is 0, pos t_cap + 100 is t_cap - Tq, count -1
    is 0, count Tq + 7 is Tq; a page id out of range is clamped into the pool."""
    N, hs, dv, Tq, dtype = 2, 64, 128, 5, torch.bfloat16
    q, k, v, coef, kb, vb, sc = _inputs(N, hs, dv)
    qd, kd, vd, cd = q[:, :Tq].to(DEV, dtype), k.to(DEV, dtype), v.to(DEV, dtype), coef.to(DEV)
    want = ops.diff_attention_decode_rows(qd, kd, vd, cd, _i32([0, CAP - Tq, 300]), _i32([Tq, Tq, 0]))
    got = ops.diff_attention_decode_rows(qd, kd, vd, cd, _i32([-5, CAP + 100, 300]), _i32([Tq + 7, Tq, -1]))
    assert torch.equal(got, want)
    full = [CAP] * B
    k_pool, v_pool, table, _, _ = PG._paginate(kd, vd, full, P, CAP, seed=1)
    n_pages = k_pool.shape[0]
    f8 = F8._paginate(kb, vb, sc, full, P, CAP, seed=2)
    pos = _i32([100, 0, CAP - Tq])
    for rows, pool, tbl in ((ops.diff_attention_decode_rows_paged, (k_pool, v_pool), table),
                            (ops.diff_attention_decode_rows_paged_fp8, f8[:3], f8[3])):
        clamped, wild = tbl.clone(), tbl.clone()
        clamped[0, 0], clamped[2, 3] = 0, n_pages - 1
        wild[0, 0], wild[2, 3] = -7, n_pages + 1000
        assert torch.equal(rows(qd, *pool, cd, wild, pos), rows(qd, *pool, cd, clamped, pos))


def test_sequences_are_independent_bitwise():
    N, hs, dv, Tq, dtype = 2, 64, 128, 8, torch.float16
    counts = _counts(Tq)
    qd, cd, contig, paged, f8 = _caches(dtype, N, hs, dv, Tq)
    got = _rows_all(qd, cd, contig, paged, f8, _i32(POS), _i32(counts))
    for b in range(B):
        sl = slice(b, b + 1)
        one = _rows_all(qd[sl], cd, (contig[0][sl], contig[1][sl]), (paged[0], paged[1], paged[2][sl].contiguous()),
                        (f8[0], f8[1], f8[2], f8[3][sl].contiguous()), _i32(POS[sl]), _i32(counts[sl]))
        for g, o in zip(got, one):
            assert torch.equal(g[sl], o), b


def test_rows_contract():
    N, hs, dv = 2, 64, 128
    q, k, v, coef = (t.to(DEV) for t in _inputs(N, hs, dv)[:4])
    pos = _i32(POS)
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_rows(torch.cat([q, q[:, :1]], dim=1), k, v, coef, pos)          # Tq = 9
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_rows(q[:, :0], k, v, coef, pos)                                 # Tq = 0
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_rows(q, k, v, coef, pos.long())
    with pytest.raises(RuntimeError):                                                             # no split plan
        ops.diff_attention_decode_rows(torch.zeros(B, 4, H, 2, 16, device=DEV), torch.zeros(B, 64, H, 2, 16, device=DEV),
                                       torch.zeros(B, 64, H, 32, device=DEV), coef, pos)
    assert not ops.decode_rows_supported(torch.float32, 16, 2, 32, 4)
    assert not ops.decode_rows_supported(torch.float32, 64, 2, 128, 9)
    assert not ops.decode_rows_supported(torch.float32, 64, 2, 64, 4)           # dv = hs only with one branch
    assert ops.decode_rows_supported(torch.float16, 128, 4, 256, 4, fp8=True)


# ------------------------------------------------------------- model level ---
class _Spy:
    """Counts the calls of the attention ops the paged step can take."""
    NAMES = {"rows": ("diff_attention_decode_rows", "diff_attention_decode_rows_paged",
                      "diff_attention_decode_rows_paged_fp8"),
             "decode": ("diff_attention_decode_ragged", "diff_attention_decode_paged", "diff_attention_decode_paged_fp8"),
             "extend": ("diff_attention_extend_ragged", "diff_attention_extend_paged", "diff_attention_extend_paged_fp8")}

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for kind, names in self.NAMES.items():
            for name in names:
                monkeypatch.setattr(ops, name, self._wrap(kind, getattr(ops, name)))

    def _wrap(self, kind, fn):
        def call(*a, _rows=False, **kw):
            if not _rows:                          # the rows ops run the extend ops' checks: count the outer call only
                self.n[kind] += 1
            return fn(*a, _rows=_rows, **kw) if kind == "extend" else fn(*a, **kw)
        return call


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"])
def test_dispatch_counts(kv_dtype, monkeypatch):
    model = PG._model("diff")
    prompts = PG._prompts(3, [5, 17, 30])
    new = torch.randint(0, 97, (3, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    cache = kv_cache.PagedKVCache(8, 32, kv_dtype=kv_dtype, rows_decode=True)
    with torch.no_grad():
        ids, _ = kv_cache.prefill_paged(model, prompts, cache)
        spy = _Spy(monkeypatch)
        kv_cache.append_paged(model, ids, new, [5, 2, 5], cache, all_rows=True)
        assert spy.n == {"rows": len(model.blocks), "decode": 0, "extend": 0}, spy.n
        kv_cache.decode_paged(model, ids, new[:, :1], cache)
        assert spy.n == {"rows": len(model.blocks), "decode": len(model.blocks), "extend": 0}, spy.n


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_fp8_pool_logits_equal_the_per_row_path_bitwise(which):
    """Only the attention op differs, and it is bitwise the same."""
    model = PG._model(which)
    prompts = PG._prompts(5, [5, 17, 30])
    g = torch.Generator().manual_seed(6)
    new = torch.randint(0, 97, (3, 5), generator=g).to(DEV)
    tok = torch.randint(0, 97, (3, 1), generator=g).to(DEV)
    out = []
    with torch.no_grad():
        for flag in (False, True):
            cache = kv_cache.PagedKVCache(8, 32, kv_dtype="fp8_e4m3", rows_decode=flag)
            ids, _ = kv_cache.prefill_paged(model, prompts, cache)
            rows = kv_cache.append_paged(model, ids, new, [5, 0, 3], cache, all_rows=True)
            out.append((rows, kv_cache.decode_paged(model, ids, tok, cache)))
    assert torch.equal(out[0][0][0], out[1][0][0]) and torch.equal(out[0][0][2, :3], out[1][0][2, :3]), which
    assert torch.equal(out[0][1], out[1][1]), which


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
@pytest.mark.parametrize("paged", [False, True])
def test_16_bit_caches_match_the_extend_path_then_truncate(which, paged):
    """Logits with the flag against the default (extend kernel), within the tolerance
    test_ragged_steps_match_full_forward uses against the full forward (1e-4); then truncate and
    continue as test_truncate_rolls_back_bitwise: bit for bit a cache that never saw the rows."""
    model = R._model(which)
    seqs = R._prompts(7)
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, 97, (3, 1), generator=g).to(DEV)
    spec = torch.randint(0, 97, (3, 4), generator=g).to(DEV)

    def run(flag, append):
        if paged:
            cache = kv_cache.PagedKVCache(12, 32, rows_decode=flag)
            ids, _ = kv_cache.prefill_paged(model, seqs, cache)
            rows = kv_cache.append_paged(model, ids, spec, [4, 4, 4], cache, all_rows=True) if append else None
            if append:
                for q, n in zip(ids, R.PROMPT_LENS):
                    cache.truncate(q, n)
            return rows, kv_cache.decode_paged(model, ids, tok, cache)
        cache = kv_cache.RaggedKVCache(rows_decode=flag)
        kv_cache.prefill_ragged(model, seqs, cache)
        rows = kv_cache.append_ragged(model, spec, [4, 4, 4], cache, all_rows=True) if append else None
        if append:
            cache.truncate(R.PROMPT_LENS)
        return rows, kv_cache.decode_ragged(model, tok, cache)

    with torch.no_grad():
        _, want = run(False, False)
        base, _ = run(False, True)
        rows, got = run(True, True)
    for b in range(3):
        assert rel_err(rows[b], base[b]) <= 1e-4, (which, paged, b)
    assert torch.equal(got, want), (which, paged)
