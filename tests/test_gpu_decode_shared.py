"""Shared-prefix decode on the paged cache (``ops.diff_attention_decode_paged_shared(_fp8)``).

Every comparison is ``torch.equal`` against ``ops.diff_attention_decode_paged(_fp8)`` on identical
inputs, at the smallest shape that has three 256-key chunks: B 5, H 2, t_cap 768, page sizes 32
and 256.  Group (0, 2, 3) shares 544 rows at page size 32 (covered to 512: two chunks; 512 rows
at page size 256) under lengths 545, 600, 768; group (1, 4) shares exactly 256 rows under lengths
257 and 256, so one member has no row of its own.  Every pool is poisoned where no sequence may
read: pages nobody reaches, rows at or past a length, table entries past a last page.  Then
groups larger than a pass, the plan's edge cases, the 512-key chunk plan, the clamps of the
device values, and the model-level dispatch behind ``shared_decode=True``."""
import functools

import pytest
import torch

import test_gpu_ragged as R
from _poison import poisoned_allocations
from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import kv_cache, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = R.TOL                       # test_gpu_decode_rows.py's (test_decode_ragged_matches_oracle's)
DTYPES = R.DTYPES
H, CAP = 2, 768
LENGTHS = (545, 257, 600, 768, 256)
GROUPS = ((0, 2, 3), (1, 4))
SHAPES = [(n, hs, dv) for hs, dv in ((32, 64), (64, 128), (128, 256)) for n in (1, 2, 3, 4)] + [(1, 64, 64)]
NAN = float("nan")


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _shared_pages(P):
    """Rows of whole pages each group of GROUPS has in common: 544 and 256 at P = 32, 512 and 256 at P = 256."""
    return (544 // P * P, 256)


@functools.lru_cache(maxsize=None)
def _logical(N, hs, dv, lengths, groups, shared, heads=H, seed=0):
    """Host rows of every sequence, made once per case and shared: members of a group hold the
    first member's first ``shared`` rows.  Returns (q, k, v, coef) in fp32."""
    B, rows = len(lengths), max(lengths)
    g = torch.Generator().manual_seed(31 * N + hs + dv + seed)
    q = torch.randn(B, heads, N, hs, generator=g)
    k = torch.randn(B, rows, heads, N, hs, generator=g)
    v = torch.randn(B, rows, heads, dv, generator=g)
    coef = torch.randn(heads, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    for members, n in zip(groups, shared):
        for b in members[1:]:
            k[b, :n] = k[members[0], :n]
            v[b, :n] = v[members[0], :n]
    return q, k, v, coef


def _pools(k, v, P, cap, lengths, groups, shared, dtype=None, seed=0):
    """Cut the logical rows into pages placed at random in a pool; the pages wholly below a group's
    shared rows exist once, named by every member's table.  Everything no sequence may read is
    poison: three pages nobody names, the rows at or past a length inside a reached page (NaN;
    fp8: byte 0x7F and NaN scales), table entries past a sequence's last page (-1) -- the first
    member of a group included, whose table the group pass reads.
    ``dtype`` None: the fp8 pools (k_u8, v_u8, scales, table); else (k_pool, v_pool, table)."""
    B, heads, N = len(lengths), k.shape[2], k.shape[3]
    owner = {}
    for members, n in zip(groups, shared):
        for b in members[1:]:
            owner[b] = (members[0], n)
    ids, table = {}, torch.full((B, cap // P), -1, dtype=torch.int32)
    need = [(b, pi) for b in range(B) for pi in range(-(-lengths[b] // P))]
    keys = []
    for b, pi in need:
        src, n = owner.get(b, (b, 0))
        key = (src, pi) if (pi + 1) * P <= n else (b, pi)
        if key not in ids:
            ids[key] = len(ids)
            keys.append(key)
        table[b, pi] = ids[key]
    n_phys = len(ids) + 3
    perm = torch.randperm(n_phys, generator=torch.Generator().manual_seed(seed + P))
    table = torch.where(table >= 0, perm[table.clamp(min=0).long()].to(torch.int32), table)
    if dtype is None:
        kb, ks = ops.kv_quant_reference(k)
        vb, vs = ops.kv_quant_reference(v)
        sc = torch.cat([ks, vs[..., None]], dim=-1)
        k_pool = torch.full((n_phys, P) + tuple(k.shape[2:]), 0x7F, dtype=torch.uint8)
        v_pool = torch.full((n_phys, P) + tuple(v.shape[2:]), 0x7F, dtype=torch.uint8)
        s_pool = torch.full((n_phys, P, heads, N + 1), NAN)
    else:
        kb, vb = k.to(dtype), v.to(dtype)
        k_pool = torch.full((n_phys, P) + tuple(k.shape[2:]), NAN, dtype=dtype)
        v_pool = torch.full((n_phys, P) + tuple(v.shape[2:]), NAN, dtype=dtype)
    for (b, pi) in keys:
        pg = int(perm[ids[(b, pi)]])
        n = min(P, lengths[b] - pi * P)
        k_pool[pg, :n] = kb[b, pi * P:pi * P + n]
        v_pool[pg, :n] = vb[b, pi * P:pi * P + n]
        if dtype is None:
            s_pool[pg, :n] = sc[b, pi * P:pi * P + n]
    if dtype is None:
        return k_pool.to(DEV), v_pool.to(DEV), s_pool.to(DEV), table.to(DEV)
    return k_pool.to(DEV), v_pool.to(DEV), table.to(DEV)


def _both(q, coef, pools, lengths, plan):
    """(shared op, paged op) on identical inputs; 3 pool tensors: 16-bit, 4: fp8."""
    ln = _i32(lengths)
    # the shared op's output and workspace are fresh NaN-filled buffers between guard bands: a
    # partial no pass wrote cannot be a stale (correct) one of an earlier call
    with poisoned_allocations() as s:
        if len(pools) == 3:
            got = ops.diff_attention_decode_paged_shared(q, *pools[:2], coef, pools[2], ln, plan)
        else:
            got = ops.diff_attention_decode_paged_shared_fp8(q, *pools[:3], coef, pools[3], ln, plan)
        s.check()
    if len(pools) == 3:
        return got, ops.diff_attention_decode_paged(q, *pools[:2], coef, pools[2], ln)
    return got, ops.diff_attention_decode_paged_fp8(q, *pools[:3], coef, pools[3], ln)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.isfinite(got.float()).all() and torch.isfinite(want.float()).all(), what
    bad = [b for b in range(got.shape[0]) if not torch.equal(got[b], want[b])]
    assert not bad, (what, "sequences that differ from the paged op", bad)


@functools.lru_cache(maxsize=None)
def _want(N, hs, dv, P):
    """The oracle's last row of the causal forward over each sequence's rows (fp64)."""
    q, k, v, coef = _logical(N, hs, dv, LENGTHS, GROUPS, _shared_pages(P))
    dt = torch.float64
    want = torch.zeros(len(LENGTHS), H, dv, dtype=dt)
    for b, L in enumerate(LENGTHS):
        for h in range(H):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs, dtype=dt)
                rows[0, L - 1] = q[b, h, i].to(dt)
                qs.append(rows)
            o = O.diff_core(qs, [k[b:b + 1, :L, h, i].to(dt) for i in range(N)], v[b:b + 1, :L, h].to(dt), coef[h].to(dt))
            want[b, h] = o[0, L - 1]
    return want


@pytest.mark.parametrize("P", [32, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", SHAPES)
def test_shared_equals_the_paged_decode_bitwise(dtype, N, hs, dv, P):
    assert ops.decode_shared_supported(dtype, hs, N, dv) and ops.decode_shared_supported(dtype, hs, N, dv, fp8=True)
    shared = _shared_pages(P)
    q, k, v, coef = _logical(N, hs, dv, LENGTHS, GROUPS, shared)
    qd, cd, B = q.to(DEV, dtype), coef.to(DEV), len(LENGTHS)
    plan = ops.shared_decode_plan(GROUPS, shared, B, DEV)
    none = ops.shared_decode_plan(GROUPS, (200, 200), B, DEV)        # below one chunk: every chunk falls to the own pass
    for name, pools in (("16-bit", _pools(k, v, P, CAP, LENGTHS, GROUPS, shared, dtype)),
                        ("fp8", _pools(k, v, P, CAP, LENGTHS, GROUPS, shared))):
        got, want = _both(qd, cd, pools, LENGTHS, plan)
        _same(got, want, (name, dtype, N, hs, dv, P))
        _same(_both(qd, cd, pools, LENGTHS, none)[0], want, (name, "200 shared rows", dtype, N, hs, dv, P))
        if name == "16-bit":
            g = got.view(B, H, dv).float().cpu()
            for b in range(B):
                err = rel_err(g[b], _want(N, hs, dv, P)[b])
                print(f"decode_shared {dtype} N={N} hs={hs} dv={dv} P={P} len={LENGTHS[b]}: rel_err {err:.3e}")
                assert err <= TOL[dtype], (dtype, N, hs, dv, P, b)


@pytest.mark.parametrize("N,fp8", [(4, False), (3, True)])
def test_groups_larger_than_a_pass(N, fp8):
    """8 members: two passes of 4 rows at N 4 on bf16 pages, four passes of 2 at N 3 on fp8 pages;
    a ninth sequence in no group."""
    hs, dv, P, dtype = 64, 128, 64, torch.bfloat16
    lengths = (530, 513, 768, 600, 512, 700, 641, 555, 300)
    groups, shared = ((0, 1, 2, 3, 4, 5, 6, 7),), (512,)
    q, k, v, coef = _logical(N, hs, dv, lengths, groups, shared, seed=1)
    pools = _pools(k, v, P, CAP, lengths, groups, shared, None if fp8 else dtype, seed=1)
    plan = ops.shared_decode_plan(groups, shared, len(lengths), DEV)
    _same(*_both(q.to(DEV, dtype), coef.to(DEV), pools, lengths, plan), (N, fp8))
    # five members with gaps between them: the passes meet empty slots
    gaps = ops.SharedDecodePlan(len(lengths), [], [], _i32([[-1, 7, -1, 2, 0, -1, 5, 3]]), _i32([512]))
    _same(*_both(q.to(DEV, dtype), coef.to(DEV), pools, lengths, gaps), (N, fp8, "gaps"))


def test_plan_edge_cases():
    N, hs, dv, P, dtype = 2, 64, 128, 32, torch.bfloat16
    shared = _shared_pages(P)
    q, k, v, coef = _logical(N, hs, dv, LENGTHS, GROUPS, shared)
    qd, cd, B = q.to(DEV, dtype), coef.to(DEV), len(LENGTHS)
    for pools in (_pools(k, v, P, CAP, LENGTHS, GROUPS, shared, dtype), _pools(k, v, P, CAP, LENGTHS, GROUPS, shared)):
        _same(*_both(qd, cd, pools, LENGTHS, ops.shared_decode_plan([], [], B, DEV)), "G = 0")
        _same(*_both(qd, cd, pools, LENGTHS, ops.shared_decode_plan([GROUPS[0]], [0], B, DEV)), "rows 0")
        # an empty batch: valid, nothing launched
        empty = ops.shared_decode_plan([], [], 0, DEV)
        tail = (pools[-1][:0], _i32(LENGTHS)[:0], empty)
        if len(pools) == 3:
            out = ops.diff_attention_decode_paged_shared(qd[:0], *pools[:2], cd, *tail)
        else:
            out = ops.diff_attention_decode_paged_shared_fp8(qd[:0], *pools[:3], cd, *tail)
        assert out.shape == (0, H * dv)
    with pytest.raises(RuntimeError):
        ops.diff_attention_decode_paged_shared(qd, *pools[:2], cd, pools[-1], _i32(LENGTHS), None)
    with pytest.raises(RuntimeError):                                # a plan made for another batch
        _both(qd, cd, _pools(k, v, P, CAP, LENGTHS, GROUPS, shared, dtype), LENGTHS, ops.shared_decode_plan([], [], B + 1, DEV))


def test_wide_chunk_plan_bitwise():
    """ceil(t_cap / 256) * H * B >= 8192: the 512-key chunk plan, built as
    test_gpu_decode_rows.test_wide_chunk_plan_bitwise builds it, over a pool of a few pages.  One
    group whose 640 shared rows cross the 512 boundary: covered to 512, one chunk."""
    Bw, Hw, N, hs, dv, cap, P, dtype = 8, 16, 2, 32, 64, 32768, 64, torch.bfloat16
    assert -(-cap // 256) * Hw * Bw >= 8192
    lengths = (700, 1030, 641, 3, 1088, 512, 640, 900)
    groups, shared = ((0, 2, 4, 6, 7),), (640,)
    q, k, v, coef = _logical(N, hs, dv, lengths, groups, shared, heads=Hw, seed=2)
    plan = ops.shared_decode_plan(groups, shared, Bw, DEV)
    for pools in (_pools(k, v, P, cap, lengths, groups, shared, dtype, seed=2), _pools(k, v, P, cap, lengths, groups, shared, seed=2)):
        _same(*_both(q.to(DEV, dtype), coef.to(DEV), pools, lengths, plan), "wide")


def test_device_values_are_clamped():
    """Only values whose clamped result is well defined: rows far past a length are the shortest
    member's length (group (1, 4): 256, what it truly shares; group (0, 2, 3): 545, covered to 512
    of its 544), a member index of B or of -7 is an empty slot, negative rows are 0."""
    N, hs, dv, P, dtype = 2, 64, 128, 32, torch.bfloat16
    shared = _shared_pages(P)
    q, k, v, coef = _logical(N, hs, dv, LENGTHS, GROUPS, shared)
    qd, cd, B = q.to(DEV, dtype), coef.to(DEV), len(LENGTHS)
    members = _i32([[0, B, 2, -7, 3, -1, -1, -1], [1, 4, -1, -1, -1, -1, -1, -1], [B, -7, -1, -1, -1, -1, -1, -1]])
    for rows in ([100000, 100000, 300], [544, -5, 0], [-2147483648, 2147483647, 7]):
        plan = ops.SharedDecodePlan(B, [], [], members, _i32(rows))
        for pools in (_pools(k, v, P, CAP, LENGTHS, GROUPS, shared, dtype), _pools(k, v, P, CAP, LENGTHS, GROUPS, shared)):
            _same(*_both(qd, cd, pools, LENGTHS, plan), rows)


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"])
def test_generate_paged_with_shared_decode(kv_dtype, monkeypatch):
    """Two prompts of 300 and 270 tokens, four samples each, page size 32: the samples of a prompt
    share its 9 and 8 full pages.  Same tokens and, step by step, the same logits bit for bit;
    the shared op ran in every layer of every step with two groups of 4 whose rows stay the
    prompts' (the samples' own tails never join them)."""
    torch.manual_seed(0)
    model = D.DiffTransformer(512, 256, 2, 2, 512, 0).to(DEV, torch.bfloat16).eval()
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in (300, 270)]
    logits, plans = {True: [], False: []}, []
    real_decode = kv_cache.decode_paged
    name = "diff_attention_decode_paged_shared" + ("" if kv_dtype is None else "_fp8")
    real_op = getattr(ops, name)

    def counted(*a, **k):
        plans.append(a[-1])
        return real_op(*a, **k)
    monkeypatch.setattr(ops, name, counted)
    outs = {}
    for flag in (False, True):
        def decode(model, seqs, tok, cache, active=None):
            out = real_decode(model, seqs, tok, cache, active)
            logits[cache.shared_decode].append(out)
            return out
        monkeypatch.setattr(kv_cache, "decode_paged", decode)
        torch.manual_seed(11)
        outs[flag] = kv_cache.generate_paged(model, prompts, 6, n_samples=4, page_size=32, kv_dtype=kv_dtype, shared_decode=flag)
    assert len(logits[True]) == len(logits[False]) == 5
    for step, (a, b) in enumerate(zip(logits[True], logits[False])):
        assert torch.equal(a, b), step
    for a, b in zip(outs[True], outs[False]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert len(plans) == 2 * 5                                       # every layer of every step, and only with the flag
    for plan in plans:
        assert plan.groups == [(0, 1, 2, 3), (4, 5, 6, 7)] and plan.shared_rows == [288, 256]
    assert len({id(p) for p in plans}) <= 2                          # rebuilt at most once: the copy on write of the first step
