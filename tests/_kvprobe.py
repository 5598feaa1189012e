"""Ill-conditioned probes for the KV-cache attention kernels (decode, extend, rows, shared).

The parity tests of this family draw q, K and V from ``randn`` and judge with ``conftest.rel_err``:
every softmax row is diffuse, every chunk and tile has nearly the same maximum, coef is far from
(1, -1), and one key skipped, doubled or leaked across the causal edge moves a row by a fraction of
a percent of the tensor's maximum.  The builders here make inputs on which those defects are not
small, and ``probe_err`` is a norm that does not pool them away.  Not a conftest; no GPU use.

Builders return a ``Case``: CPU fp32 ``q (B, Tq, H, N, hs)``, ``k (B, cap, H, N, hs)``,
``v (B, cap, H, dv)``, ``coef (H, N)``, ``pos`` (row r of sequence b sits at key pos[b] + r and sees
keys 0 .. pos[b] + r; a decode at length L is Tq = 1, pos = L - 1) and ``hot``, the planted keys.
Every query of a (b, h, branch) block is sqrt(hs) * unit(0.8 u + 0.6 g_r) around one direction u, so
a key planted along u is hot for every row that may see it -- and for the row just before it, which
may not.

* ``planted``: randn background; K_branch[j*] = gap * (direction), so its score is gap nats above the
  background's mean 0; V[j*] = +-100 per column.  gap 8: p_top ~ 0.9 at a few hundred keys; gap 40: a
  one-hot row, every other exponential underflows and one chunk / tile carries the only weight.
* ``ramp``: scores rise by ``span`` nats from key 0 to the last key in even branches and fall in odd
  ones, plus 0.3 x noise: every tile raises one branch's running maximum, the other's sits at key 0.
* ``cancelling``: coef sums to 0 -- (1, -1), (1, -0.5, -0.5), ... -- and branch i's queries are branch
  0's, its keys branch 0's plus 0.1 x noise: the output is a small difference of O(1) maps.
* ``scaled_rows``: a case re-scaled for the fp8 cache so that the stored scales span four decades
  (``logspace(-2, 2)`` permuted over rows, per head).  V rows are multiplied by them.  K rows cannot
  be (a score would move by the same factor): K is multiplied by 2^-7 and q by 2^7 (exact in every
  format), coordinate 0 of q is zeroed and coordinate 0 of K row j holds the row's scale s_j, which
  is then the row's amax and so its stored scale, without moving a score.  Planted keys sit on
  1e-2 rows between 1e+2 neighbours, or the other way round: a scale taken from the next row shows
  at four decades.

Oracle: ``oracle`` runs ``oracle.diffattn_oracle.diff_core`` in fp64 on the values as stored (the
caller rounds to the dtype, or dequantises) and returns ``want`` and the un-cancelled magnitude
``D = diff_core(q, k, |V|, |coef|) = sum_i |coef_i| A_i |V|``.  ``probe_err`` is
``max_c |got - want| / max_c D`` per (b, row, h): the forward-error norm of a signed sum, meaningful
where ``want`` is ~ 0, never pooled over rows, heads or sequences.  The bar is ``TOL[dtype]`` on
every block.  ``_bands.reference_algorithm`` is not the yardstick here: it rounds scores in the
dtype, and a score of 30 rounded at 2^-8 costs it 3.5e-2 on the bf16 ramp; the kernels keep fp32
scores.
"""
import types

import torch

from oracle import diffattn_oracle as O

TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 2e-2}
GAPS = (8.0, 40.0)
SPAN = 30.0
V_HOT = 100.0


def trained_coef(H, N):
    """(1, -lambda, +lambda', ...) with lambda near 1, another one per head."""
    c = torch.tensor([[(-1.0) ** i * (1.0 - 0.1 * i - 0.03 * h) for i in range(N)] for h in range(H)])
    c[:, 0] = 1.0
    if N > 1:
        c[:, 1] = -(0.95 - 0.03 * torch.arange(H))
    return c


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _background(dims, cap, pos, seed, shared_u=False):
    B, Tq, H, N, hs, dv = dims
    g = torch.Generator().manual_seed(seed)
    u = _unit(torch.randn(B, 1, H, N, hs, generator=g))
    if shared_u:
        u = u[:1].expand(B, 1, H, N, hs).contiguous()
    q = hs ** 0.5 * _unit(0.8 * u + 0.6 * _unit(torch.randn(B, Tq, H, N, hs, generator=g)))
    k = torch.randn(B, cap, H, N, hs, generator=g)
    v = torch.randn(B, cap, H, dv, generator=g)
    assert all(0 <= p and p + Tq <= cap for p in pos) and len(pos) == B
    return g, u, types.SimpleNamespace(q=q, k=k, v=v, coef=trained_coef(H, N), pos=tuple(pos), Tq=Tq, cap=cap,
                                       dims=dims, hot=[], kind=None)


def planted(dims, cap, pos, spots, seed, shared_u=False):
    """``spots``: {(b, h): [(where, branch, gap), ...]}.  ``where``: a key index (K[j] = gap / 0.8 * u,
    hot for every row of the block), ``"own"`` (K[pos + r] = gap * unit(q_r) for every row r: the
    row's own key) or ``"next"`` (K[pos + r + 1] = gap * unit(q_r): the key just past row r's causal
    edge, the first invisible key for the last row; it must fit the capacity)."""
    g, u, c = _background(dims, cap, pos, seed, shared_u)
    B, Tq, H, N, hs, dv = dims
    for (b, h), plants in sorted(spots.items()):
        for where, i, gap in plants:
            if isinstance(where, int):
                keys, rows = [where], [u[b, 0, h, i] * (gap / 0.8)]
            else:
                off = {"own": 0, "next": 1}[where]
                keys = [pos[b] + r + off for r in range(Tq)]
                rows = [_unit(c.q[b, r, h, i]) * gap for r in range(Tq)]
            for j, row in zip(keys, rows):
                assert 0 <= j < cap, (j, cap)
                c.k[b, j, h, i] = row
                c.v[b, j, h] = V_HOT * (torch.randint(0, 2, (dv,), generator=g) * 2.0 - 1.0)
                c.hot.append((b, j, h, i, gap))
    c.kind = "planted"
    return c


def ramp(dims, cap, pos, seed, span=SPAN, shared_u=False):
    g, u, c = _background(dims, cap, pos, seed, shared_u)
    B, Tq, H, N, hs, dv = dims
    last = max(pos) + Tq - 1
    t = (torch.arange(cap, dtype=torch.float32) / max(last, 1)).clamp(max=1.0)
    for i in range(N):
        ti = t if i % 2 == 0 else 1.0 - t
        c.k[:, :, :, i] = 0.3 * c.k[:, :, :, i] + (span / 0.8) * ti[None, :, None, None] * u[:, :, :, i]
    c.kind = "ramp"
    return c


def cancelling(dims, cap, pos, seed, shared_u=False):
    g, u, c = _background(dims, cap, pos, seed, shared_u)
    B, Tq, H, N, hs, dv = dims
    assert N >= 2, "one branch has nothing to cancel against"
    c.coef = torch.tensor([[1.0] + [-1.0 / (N - 1)] * (N - 1)] * H)
    noise = torch.randn(B, cap, H, N, hs, generator=g)
    for i in range(1, N):
        c.q[:, :, :, i] = c.q[:, :, :, 0]
        c.k[:, :, :, i] = c.k[:, :, :, 0] + 0.1 * noise[:, :, :, i]
    c.kind = "cancelling"
    return c


def scaled_rows(case, seed, flip=False):
    """See the module docstring.  ``flip``: planted keys on 1e+2 rows between 1e-2 neighbours."""
    B, Tq, H, N, hs, dv = case.dims
    g = torch.Generator().manual_seed(seed)
    s = torch.stack([torch.logspace(-2, 2, case.cap)[torch.randperm(case.cap, generator=g)] for _ in range(B * H)])
    s = s.view(B, H, case.cap).permute(0, 2, 1).contiguous()                 # (B, cap, H)
    lo, hi = (1e2, 1e-2) if flip else (1e-2, 1e2)
    for b, j, h, _, _ in case.hot:
        for n in (j - 1, j + 1):
            if 0 <= n < case.cap:
                s[b, n, h] = hi
    for b, j, h, _, _ in case.hot:
        s[b, j, h] = lo
    out = types.SimpleNamespace(**vars(case))
    out.q = case.q * 128.0
    out.q[..., 0] = 0.0
    out.k = case.k / 128.0
    out.k[..., 0] = s[..., None]
    out.v = case.v * s[..., None]
    out.scales = s
    return out


def stored(case, dtype):
    """(q, k, v) as a 16- or 32-bit cache of ``dtype`` holds them."""
    return case.q.to(dtype), case.k.to(dtype), case.v.to(dtype)


def stored_fp8(case, dtype, quant):
    """``quant``: ``ops.kv_quant_reference``.  Returns q in ``dtype``, the bytes and scales
    (kb, vb, sc (B, cap, H, N + 1)) and the fp32 rows they dequantise to (exact: byte * scale)."""
    N = case.dims[3]
    kb, ks = quant(case.k)
    vb, vs = quant(case.v)
    sc = torch.cat([ks, vs[..., None]], dim=-1)
    k = kb.view(torch.float8_e4m3fn).float() * sc[..., :N, None]
    v = vb.view(torch.float8_e4m3fn).float() * sc[..., N, None]
    return case.q.to(dtype), kb, vb, sc, k, v


def oracle(q, k, v, coef, pos, counts=None, abs_only=False):
    """fp64 ``diff_core`` on the values given, per sequence over its first pos[b] + count rows, rows
    pos[b]: kept.  q (B, Tq, H, N, hs), k (B, >= L, H, N, hs), v (B, >= L, H, dv), coef (H, N).
    Returns (want, D), each (B, Tq, H, dv), zeros in rows >= counts[b]."""
    B, Tq, H, N, hs = q.shape
    dt = torch.float64
    want = torch.zeros(B, Tq, H, v.shape[-1], dtype=dt)
    D = torch.zeros_like(want)
    cf = coef.to(dt).t()[:, :, None, None].contiguous()                     # (N, H, 1, 1): one batch entry per head
    for b in range(B):
        n = Tq if counts is None else counts[b]
        if n == 0:
            continue
        L = pos[b] + n
        qs, ks = [], []
        for i in range(N):
            rows = torch.zeros(H, L, hs, dtype=dt)
            rows[:, pos[b]:] = q[b, :n, :, i].to(dt).transpose(0, 1)
            qs.append(rows)
            ks.append(k[b, :L, :, i].to(dt).transpose(0, 1))
        vv = v[b, :L].to(dt).transpose(0, 1)
        D[b, :n] = O.diff_core(qs, ks, vv.abs(), cf.abs())[:, pos[b]:].transpose(0, 1)
        if not abs_only:
            want[b, :n] = O.diff_core(qs, ks, vv, cf)[:, pos[b]:].transpose(0, 1)
    return want, D


def probe_err(got, want, D):
    """max_c |got - want| / max_c D per (b, row, h); 0 where D is 0 and got equals want (padding)."""
    got, want, D = (torch.as_tensor(t).double().cpu() for t in (got, want, D))
    assert got.shape == want.shape == D.shape, (got.shape, want.shape, D.shape)
    num, den = (got - want).abs().amax(-1), D.amax(-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))


def p_top(case):
    """Softmax weight of each planted key in its own branch, for the last row that sees it first
    (fp64 from the fp32 builders' values): [(b, j, h, i, gap, p)]."""
    out = []
    B, Tq, H, N, hs, dv = case.dims
    for b, j, h, i, gap in case.hot:
        r = min(max(j - case.pos[b], 0), Tq - 1)
        L = case.pos[b] + r + 1
        if j >= L:
            continue
        s = (case.k[b, :L, h, i].double() @ case.q[b, r, h, i].double()) / hs ** 0.5
        out.append((b, j, h, i, gap, torch.softmax(s, 0)[j].item()))
    return out
