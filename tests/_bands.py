"""Band-resolved parity along the sequence axis.

``rel_err`` (conftest.py) divides a tensor's largest error by the tensor's
largest oracle value.  Under a causal mask |O[t]| falls like 1/sqrt(t) and dK[j], dV[j] sum over
the T - j later queries only, so that denominator comes from the first few rows and the late
rows -- after the K/V ring has wrapped many times, in the ragged last tile, with the online
softmax statistics carried over every tile -- may be wrong by a large fraction of themselves
without moving the norm.  This module takes the same norm over *bands* of rows instead:
octaves below 64 (where the magnitudes change fastest), then the kernels' 64-row tiles, the
last one ragged, each band kept apart per batch, head and (for dQ / dK) branch.

Single rows are ill conditioned (row 0's dQ is exactly zero, row 1's is small by cancellation)
and a flat 2e-2 has no headroom once the norm is band-local, so the bar of one tensor is
``max(TOL, 2 x the reference algorithm's own worst band error)``: ``reference_algorithm`` runs
the reference project's forward in the kernel's dtype on the CPU, torch autograd its backward.
The bar never reads the kernel's output.  Not a conftest: tests import what they need.
"""
import math
import types

import torch

from oracle import diffattn_oracle as orc

TILE = 64           # the attention kernels' tile stride along the sequence
FACTOR = 2.0        # the project's margin over the reference algorithm (test_gpu_parity._long_case ref_bar)


def row_bands(T):
    """[0,1) [1,2) [2,4) ... [32,64), then 64-row tiles, the last one ragged: every row of
    range(T) once, in order."""
    edges = [0, 1, 2, 4, 8, 16, 32] + list(range(TILE, T + TILE, TILE))
    return [(lo, min(hi, T)) for lo, hi in zip(edges, edges[1:]) if lo < T]


def sampled_bands(rows, T, least=2, uncounted=()):
    """``row_bands(T)`` over the sorted sample ``rows``: index ranges into ``rows``, a band that
    holds fewer than ``least`` sampled rows merged into its neighbour (the next one; the last
    into the one before).  Rows in ``uncounted`` stay in their band but do not count towards
    ``least``: dQ's row 0 is exactly zero in the oracle, so a band of rows {0, 1} would stand on
    row 1 alone -- a single row, small by cancellation, which no rounding algorithm matches
    relative to itself (the reference algorithm's own error there was 0.008 ... 0.8 from one
    (b, h) to the next at the suite's full shapes)."""
    assert list(rows) == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < T
    out, lo, n, counted = [], 0, 0, 0
    for b_lo, b_hi in row_bands(T):
        n += sum(b_lo <= r < b_hi for r in rows)
        counted += sum(b_lo <= r < b_hi and r not in uncounted for r in rows)
        if counted >= least:
            out.append((lo, n))
            lo, counted = n, 0
    if lo < len(rows):
        if out:
            out[-1] = (out[-1][0], len(rows))
        else:
            out.append((0, len(rows)))
    return out


def band_max(x, row_dim, groups, bands=None):
    """max|x| over each (band x group) block: shape (len(bands), *[x.shape[g] for g in groups]).
    ``groups``: the axes kept apart; every other axis but ``row_dim`` is reduced with the rows."""
    x = torch.as_tensor(x).double().abs()
    bands = row_bands(x.shape[row_dim]) if bands is None else bands
    rest = [d for d in range(x.dim()) if d != row_dim and d not in groups]
    x = x.permute(row_dim, *groups, *rest).flatten(1 + len(groups)) if rest else x.permute(row_dim, *groups).unsqueeze(-1)
    return torch.stack([x[lo:hi].amax(dim=(0, -1)) for lo, hi in bands])


def band_errors(got, ref, row_dim, groups, bands=None):
    """max|got - ref| / max|ref| over each (band x group) block.  Returns ``(err, zero)``:
    ``err`` of shape (bands, *group sizes), 0 where the oracle's block is exactly zero, and
    ``zero``, the boolean map of those blocks (they have no band-local error; see
    ``zero_block_excess``)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    num = band_max(got - ref, row_dim, groups, bands)
    den = band_max(ref, row_dim, groups, bands)
    zero = den == 0
    return torch.where(zero, torch.zeros_like(num), num / den.masked_fill(zero, 1.0)), zero


def zero_block_excess(got, ref, row_dim, groups, bands=None):
    """The largest |got| inside the blocks whose oracle is exactly zero, over the tensor's
    global oracle maximum (0.0 without such blocks): to be held under TOL[dtype]."""
    _, zero = band_errors(got, ref, row_dim, groups, bands)
    if not zero.any():
        return 0.0
    top = torch.as_tensor(ref).double().abs().max().item()
    return band_max(got, row_dim, groups, bands)[zero].max().item() / (top if top > 0 else 1.0)


def worst(err, bands=None, T=None):
    """(largest error, its row range, its group index) of a ``band_errors`` map."""
    flat = int(err.flatten().argmax())
    idx = list(torch.unravel_index(torch.tensor(flat), err.shape))
    idx = [int(i) for i in idx]
    if bands is None and T is not None:
        bands = row_bands(T)
    rows = list(bands[idx[0]]) if bands is not None else idx[0]
    return err.flatten()[flat].item(), rows, idx[1:]


def bar(tol, yardstick_worst):
    """The bar of one tensor of one case: max(TOL[dtype], 2 x the reference algorithm's worst
    band error against the fp64 oracle over that tensor's bands)."""
    return max(tol, FACTOR * yardstick_worst)


MAX_GROWTH = 55 * math.log(2.0)     # the fixed-reference forward re-runs a row block beyond ~55 log2 units


class _BranchRoundedOi(torch.autograd.Function):
    """``c_i * A_i * m_i`` of one branch (A_i = softmax(s), fp32), differentiated as the kernels
    do: the softmax backward's row constant delta_i = <dO, O_i>, with O_i = (A_i m_i) V, and with
    it d(coef_i) = sum over rows of delta_i, are taken from the O_i the forward *stored*, which
    carries one rounding step the reference does not take (csrc/attn_kernels.h).  ``step``:

    - ``"obr_f16"`` (DTA_OBR_F16=1): the forward's epilogue stores the normalised O_i as fp16.
    - ``"packed_p"`` (the 16-bit forward's fixed reference maximum): after a row's
      first key tile the maximum m stays fixed, P = exp(s - m) is packed to ``dtype`` for the PV
      product while the row sum l adds the fp32 P, and O_i = (packed P) V / l.  The dominant P of
      a row is then 2^growth, not 1, and rounds by up to half an ulp of ``dtype``; in a nearly
      one-hot row O_i is off by that fraction of V_top, and dP_top - delta_i, itself only
      (1 - p_top) of dP_top, by that fraction of delta_i.

    Everything else is plain autograd: only <dO, stored O_i - O_i> is added to the exact row sum."""

    @staticmethod
    def forward(ctx, s, c_i, m, v, do, step, dtype):
        a = torch.softmax(s, dim=-1)
        am = a if m is None else a * m
        o_i = am @ v.float()
        if step == "obr_f16":
            stored = o_i.half().float()
        else:
            assert step == "packed_p", step
            top = s.amax(-1, keepdim=True)
            ref = s[..., :TILE].amax(-1, keepdim=True)
            ref = torch.where(top - ref > MAX_GROWTH, top, ref)
            p = torch.exp(s - ref)
            packed = (p if m is None else p * m).to(dtype).float()
            stored = (packed @ v.float()) / p.sum(-1, keepdim=True)
        slip = (do.float() * (stored - o_i)).sum(-1, keepdim=True)
        ctx.save_for_backward(a, am, c_i, m, slip)
        return c_i * am

    @staticmethod
    def backward(ctx, g):
        a, am, c_i, m, slip = ctx.saved_tensors
        g_a = g * c_i if m is None else g * c_i * m
        delta = (a * g_a).sum(-1, keepdim=True) + c_i * slip
        return a * (g_a - delta), (g * am).sum() + slip.sum(), None, None, None, None, None


def reference_algorithm(qkv, coef, do, H, N, hs, dv, dtype, freqs_c=None, masks=None, obr_f16=False,
                        packed_p=False):
    """The reference project's attention forward run on the CPU in ``dtype`` on the packed,
    already quantised ``qkv`` (B, T, 2 H N hs + H dv), restated from diff_transformer.py:57-72
    and Ndiff_transformer.py:102-125 as they run under train.py's autocast: the scores come from
    a ``dtype`` matmul and are scaled in ``dtype``, the softmax is fp32, the maps are combined
    with the fp32 coefficients in fp32 and the combination is cast to ``dtype`` for ``@ V``.
    RoPE (``freqs_c``) rotates in fp32 before the cast back (apply_rotary_emb,
    Ndiff_transformer.py:11-22); ``masks`` (B, H, N, T, T) are dropout multipliers m / (1 - p)
    on every softmax map (diff_transformer.py:66-67), the ones test_gpu_dropout.drop_masks
    makes.  The backward is torch autograd through exactly that graph.  fp32: the same code.
    ``obr_f16`` / ``packed_p``: one rounding step the kernels take by design and the reference
    does not, in the per-branch O_i that delta_i is made of (``_BranchRoundedOi``): O_i stored as
    fp16 on the DTA_OBR_F16=1 path; P packed to ``dtype`` against a fixed reference maximum.
    Returns (out, d qkv, d coef) as float64, shaped like the kernels' results."""
    B, T, W = qkv.shape
    nq = H * N * hs
    x = qkv.to(dtype).clone().requires_grad_(True)
    c = coef.float().clone().requires_grad_(True)
    q = x[..., :nq].view(B, T, H, N, hs)
    k = x[..., nq:2 * nq].view(B, T, H, N, hs)
    v = x[..., 2 * nq:].view(B, T, H, dv)
    future = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    outs = []
    for h in range(H):
        diff = None
        for i in range(N):
            qi, ki = q[:, :, h, i], k[:, :, h, i]
            if freqs_c is not None:
                qi, ki = orc.apply_rotary_emb(qi, freqs_c), orc.apply_rotary_emb(ki, freqs_c)
            s = ((qi @ ki.transpose(-2, -1)) * hs ** -0.5).masked_fill(future, float("-inf")).float()
            m = masks[:, h, i].float() if masks is not None else None
            if obr_f16 or packed_p:
                assert not (obr_f16 and packed_p)
                term = _BranchRoundedOi.apply(s, c[h, i], m, v[:, :, h].detach(), do.view(B, T, H, dv)[:, :, h].to(dtype),
                                              "obr_f16" if obr_f16 else "packed_p", dtype)
            else:
                a = torch.softmax(s, dim=-1)
                term = c[h, i] * (a if m is None else a * m)
            diff = term if diff is None else diff + term
        outs.append(diff.to(dtype) @ v[:, :, h])
    out = torch.cat(outs, dim=-1)
    out.backward(do.to(dtype))
    return out.detach().double(), x.grad.double(), c.grad.double()


def split(gx, H, N, hs, dv):
    """d(qkv) (B, T, W) -> dQ, dK (B, T, H, N, hs) and dV (B, T, H, dv)."""
    nq = H * N * hs
    return (gx[..., :nq].unflatten(-1, (H, N, hs)), gx[..., nq:2 * nq].unflatten(-1, (H, N, hs)),
            gx[..., 2 * nq:].unflatten(-1, (H, dv)))


GROUPS = {"O": (0, 2), "dQ": (0, 2, 3), "dK": (0, 2, 3), "dV": (0, 2)}      # batch, head[, branch]; rows: axis 1


def tensors(out, gx, H, N, hs, dv):
    """The four banded tensors of one forward + backward, rows on axis 1."""
    dq, dk, dvv = split(gx, H, N, hs, dv)
    return {"O": out.unflatten(-1, (H, dv)), "dQ": dq, "dK": dk, "dV": dvv}


def dcoef_errors(gc, ref):
    """Each d(coef) entry's error over its head's largest oracle entry (H, N), as section C of
    test_gpu_plan_matrix.py takes it."""
    ref = ref.double()
    return (gc.double() - ref).abs() / ref.abs().amax(1, keepdim=True)


def judge(got, oracle, yard, dims, tol, plain=None):
    """Band errors of the kernel's results ``got`` and of the reference algorithm's ``yard``
    against ``oracle`` (each (out, d qkv, d coef)).  Returns name -> namespace(kernel, where,
    yardstick, bar, zero, excess, plain): the kernel's worst band error, [row range, group
    index] of that band, the yardstick's worst, the bar made of it, the zero-oracle block map,
    the kernel's largest value in those blocks over the tensor's oracle maximum and -- where
    ``yard`` carries a named rounding step -- the worst band of the plain algorithm ``plain``."""
    B, T, H, N, hs, dv = dims
    res = {}
    tg, to, ty = (tensors(t[0], t[1], H, N, hs, dv) for t in (got, oracle, yard))
    tp = tensors(plain[0], plain[1], H, N, hs, dv) if plain is not None else None
    for name, groups in GROUPS.items():
        ke, zero = band_errors(tg[name], to[name], 1, groups)
        k_w, rows, grp = worst(ke, T=T)
        y_w = band_errors(ty[name], to[name], 1, groups)[0].max().item()
        p_w = band_errors(tp[name], to[name], 1, groups)[0].max().item() if tp else None
        res[name] = types.SimpleNamespace(kernel=k_w, where=[rows, grp], yardstick=y_w, bar=bar(tol, y_w), zero=zero,
                                          excess=zero_block_excess(tg[name], to[name], 1, groups), plain=p_w)
    k_w, h, i = worst(dcoef_errors(got[2], oracle[2]))
    y_w = dcoef_errors(yard[2], oracle[2]).max().item()
    p_w = dcoef_errors(plain[2], oracle[2]).max().item() if plain is not None else None
    res["dcoef"] = types.SimpleNamespace(kernel=k_w, where=[h] + i, yardstick=y_w, bar=bar(tol, y_w), zero=None,
                                         excess=0.0, plain=p_w)
    return res
