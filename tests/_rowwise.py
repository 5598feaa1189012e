"""Problems, fp64 oracles and fp32 yardsticks of the row-wise kernels (csrc/elementwise.hip).

CPU only: test_gpu_rowwise_matrix.py runs the kernels on what this module makes, and
test_rowwise_cpu.py checks the module itself (the width -> band rule, the per-row measure, the
yardsticks) without a GPU.  Not a conftest: tests import what they need.

LayerNorm rows differ in scale (a power of ten cycling over 1e-3 ... 1e3) and in offset (up to
100 x the spread), and four rows are planted: a constant row, a row of zeros, a row of N(0, 1)
with one 1e4 outlier and a row whose dy is all zero.  dx scales with a row's rstd, so under the
whole-tensor ``rel_err`` a large-spread row may be wholly wrong unseen: every activation is
judged row by row (``row_errors``: ``_bands.band_errors`` over one-row bands).

The oracle is fp64 from the inputs as quantised to the case's storage dtypes.  The yardstick is
the same operation done plainly in fp32 on the CPU (fp32 statistics, one rounding to the storage
dtype), measured against that oracle row by row; a row's bar is ``max(TOL, 2 x yardstick)``
(``_bands.bar``) and never reads a kernel's output.
"""
import types

import torch
from torch.nn import functional as F

import _bands
from oracle import diffattn_oracle as orc

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TOL = {F32: 1e-4, BF16: 2e-2, F16: 2e-2}                     # test_gpu_parity.TOL
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}

# (x / dx dtype, y / dy dtype): the three launch_ln cases and the two launch_ln_mixed ones
COMBOS = {"f32": (F32, F32), "bf16": (BF16, BF16), "f16": (F16, F16), "f32-bf16": (F32, BF16), "f32-f16": (F32, F16)}
MIXED = ("f32-bf16", "f32-f16")

# ---- the width bands of ln_launch / ln_launch_mixed, restated -------------------------------
LN_BANDS = (1, 2, 4, 8, 16)               # CH: 8-element chunks per lane of ln_fwd_kernel<*, CH>
WIDTHS = [8, 512, 520, 1024, 1032, 2048, 2056, 3072, 4096, 4104, 8192]
ROWS = [1, 9, 37, 513]
LN_MAX_BLOCKS = 512                       # kLnBwdMaxBlk


def ln_band(C):
    """The forward instantiation's CH for width C: ceil(C / 512) rounded up into LN_BANDS; None
    for a width the entry points reject (not a multiple of 8, or wider than 8192)."""
    if C <= 0 or C % 8 or C > 8192:
        return None
    ch = -(-C // 512)
    return next(b for b in LN_BANDS if ch <= b)


def ln_bwd_chb(C):
    """ln_bwd_rb_kernel<*, CHB>: CHB = (CH + 3) / 4."""
    return (ln_band(C) + 3) // 4


def ln_bwd_ring(C):
    """Register slots of raw rows in the backward's ring: prefetch depth 3 at CHB 1, else 1."""
    return 4 if ln_bwd_chb(C) == 1 else 2


def ln_bwd_blocks(rows):
    return min((rows + 7) // 8, LN_MAX_BLOCKS)


def band_edges(band):
    """The narrowest and the widest accepted width of a band."""
    lo = 8 if band == 1 else 512 * (band // 2) + 8
    return lo, 512 * band


def single_row_targets(rows, C):
    """Rows at which one nonzero dy row shows a skipped or doubled row of the backward at full
    size: 0, 1, the last, the first row past one full trip of the grid, and the last row of a
    workgroup whose row count leaves a ring slot part filled (none when every count is a
    multiple of the ring)."""
    blocks, ring = ln_bwd_blocks(rows), ln_bwd_ring(C)
    out = {0, min(1, rows - 1), rows - 1, min(blocks, rows - 1)}
    for b in range(blocks):
        n = len(range(b, rows, blocks))
        if n % ring:
            out.add(b + (n - 1) * blocks)
            break
    return sorted(out)


# ---- the per-row measure ------------------------------------------------------------------
def row_errors(got, ref):
    """max|got - ref| / max|ref| of every row of a (rows, C) tensor, and the map of the rows
    whose oracle is exactly zero (error 0 there; see ``zero_row_excess``).  ``_bands.band_errors``
    with the rows as its group axis under one band of a leading unit axis: one block per row,
    without a Python loop over the rows."""
    err, zero = _bands.band_errors(torch.as_tensor(got)[None], torch.as_tensor(ref)[None], 0, (1,), bands=[(0, 1)])
    return err[0], zero[0]


def zero_row_excess(got, ref):
    """The largest |got| in the rows whose oracle is exactly zero, over the tensor's oracle
    maximum (``_bands.zero_block_excess`` over the same one-row blocks)."""
    return _bands.zero_block_excess(torch.as_tensor(got)[None], torch.as_tensor(ref)[None], 0, (1,), bands=[(0, 1)])


def vec_err(got, ref):
    """``conftest.rel_err``: max|got - ref| / max|ref| over a whole vector."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    den = ref.abs().max().item()
    return (got - ref).abs().max().item() / (den if den > 0 else 1.0)


def judge_rows(got, oracle, yard, tol):
    """One activation of one case, row by row.  Returns namespace(kernel, where, yardstick, bar,
    excess, over): the kernel's worst row error and its row, the yardstick's worst row, the bar
    of the kernel's worst row, the kernel's largest value in zero-oracle rows over the oracle
    maximum, and the rows whose error is not under their own bar max(tol, 2 x yardstick)."""
    ke, _ = row_errors(got, oracle)
    ye, _ = row_errors(yard, oracle)
    bars = torch.clamp(_bands.FACTOR * ye, min=tol)
    w = int(ke.argmax())
    over = [(r, ke[r].item(), bars[r].item()) for r in torch.nonzero(~(ke < bars)).flatten().tolist()]
    return types.SimpleNamespace(kernel=ke[w].item(), where=w, yardstick=ye.max().item(), bar=bars[w].item(),
                                 excess=zero_row_excess(got, oracle), over=over)


def judge_vec(got, oracle, yard, tol=TOL[F32]):
    """dw / db: whole-vector error at the fp32 bar in every dtype combination (fp32 sums of
    exactly represented inputs)."""
    k = vec_err(got, oracle)
    return types.SimpleNamespace(kernel=k, where=None, yardstick=vec_err(yard, oracle), bar=tol, excess=0.0,
                                 over=[] if k < tol else [(None, k, tol)])


# ---- LayerNorm problems ---------------------------------------------------------------------
def f32(v):
    """``v`` as the kernels receive it: rounded to fp32."""
    return torch.tensor(v, dtype=F32).item()


def planted_rows(rows):
    """name -> row index of the planted rows (none below 9 rows)."""
    if rows < 9:
        return {}
    return {"const": 2, "zeros": 4, "outlier": rows - 4, "zero_dy": rows - 2}


CONST = 0.25     # the constant row's value: C x 0.25 sums exactly in fp32


def ln_problem(combo, rows, C, eps, out_scale, fused=False, seed=0):
    """Inputs (as stored), the fp64 oracle and the fp32 yardstick of one LN forward + backward.

    ``fused``: the add + LN fusion of the mixed combos (fp32 residual stream x, 16-bit branch
    output ``res``, LN of xo = x + res; backward adds the stream's gradient ``dres`` and writes
    the branch's 16-bit gradient ``da`` beside dx); out_scale is 1 there.
    Returns namespace(x, res, w, b, dy, dres, eps, out_scale, oracle, yard): ``oracle`` / ``yard``
    map y, dx, dw, db, mean, rstd (and xo, da when fused) to fp64 / the plain fp32 results."""
    xdt, ydt = COMBOS[combo]
    assert not fused or combo in MIXED
    eps, out_scale = f32(eps), f32(1.0 if fused else out_scale)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + C)
    r = torch.arange(rows)
    scale = 10.0 ** ((r % 7) - 3).double()
    off = torch.tensor([0.0, 1.0, 100.0, 10.0], dtype=torch.float64)[r % 4]
    if xdt == F16 or (fused and ydt == F16):
        off = torch.minimum(off, (3.0e4 / scale - 6).clamp(min=0))          # stay inside fp16's range
    base = torch.randn(rows, C, generator=g, dtype=torch.float64)
    x = (base + off[:, None]) * scale[:, None]
    res = None
    if fused:
        res = 0.5 * torch.randn(rows, C, generator=g, dtype=torch.float64) * scale[:, None]
    w = (1 + 0.1 * torch.randn(C, generator=g)).float()
    b = (0.3 + 0.1 * torch.randn(C, generator=g)).float()
    dy = torch.randn(rows, C, generator=g)
    plant = planted_rows(rows)
    if plant:
        x[plant["const"]] = CONST
        x[plant["zeros"]] = 0.0
        x[plant["outlier"]] = torch.randn(C, generator=g, dtype=torch.float64)
        x[plant["outlier"], (3 * C) // 4 - 1] = 1e4
        dy[plant["zero_dy"]] = 0.0
        if fused:
            for k in ("const", "zeros", "outlier"):
                res[plant[k]] = 0.0
    x, dy = x.to(xdt), dy.to(ydt)
    res = res.to(ydt) if fused else None

    # fp64 oracle from the stored inputs
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    if fused:
        r64 = res.double().requires_grad_(True)
        s64 = x64 + r64
        y64 = F.layer_norm(s64, (C,), w64, b64, eps)
    else:
        s64 = x64
        y64 = orc.group_layer_norm(s64, w64, b64, eps) * out_scale
    mean64 = s64.detach().mean(-1)
    rstd64 = 1.0 / (s64.detach().var(-1, unbiased=False) + eps).sqrt()
    dres = None
    loss = (y64 * dy.double()).sum()
    if fused:
        # the stream's own gradient, of the LN gradient's size in every row
        dres = (0.5 * torch.randn(rows, C, generator=g).double() * rstd64[:, None]).float()
        loss = loss + (s64 * dres.double()).sum()
    loss.backward()
    oracle = {"y": y64.detach(), "dx": x64.grad, "dw": w64.grad, "db": b64.grad, "mean": mean64, "rstd": rstd64}
    if fused:
        oracle.update(xo=s64.detach(), da=r64.grad)

    # the plain fp32 algorithm, one rounding to the storage dtype
    s = x.float() + res.float() if fused else x.float()
    mean = s.mean(-1, keepdim=True)
    d = s - mean
    rstd = 1.0 / ((d * d).mean(-1, keepdim=True) + eps).sqrt()
    xh = d * rstd
    y = ((xh * w + b) * out_scale).to(ydt)
    gs = dy.float() * out_scale
    gw = gs * w
    dx = rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))
    if fused:
        dx = dx + dres
    yard = {"y": y, "dx": dx.to(xdt), "dw": (gs * xh).sum(0), "db": gs.sum(0), "mean": mean[:, 0], "rstd": rstd[:, 0]}
    if fused:
        yard.update(xo=s, da=dx.to(ydt))
    return types.SimpleNamespace(combo=combo, rows=rows, C=C, x=x, res=res, w=w, b=b, dy=dy, dres=dres, eps=eps,
                                 out_scale=out_scale, fused=fused, oracle=oracle, yard=yard, plant=plant)


def ln_tols(combo):
    """tensor name -> its bar's floor: the storage dtype's TOL for the activations."""
    xdt, ydt = COMBOS[combo]
    return {"y": TOL[ydt], "dx": TOL[xdt], "xo": TOL[F32], "da": TOL[ydt]}


def stat_errors(pb, mean, rstd):
    """mean and rstd of every row against the oracle: the mean's error in units of the row's
    sqrt(var + eps) (what an error of the mean costs the normalised row), rstd's relative."""
    o = pb.oracle
    em = ((torch.as_tensor(mean).double().cpu() - o["mean"]).abs() * o["rstd"]).max().item()
    er = ((torch.as_tensor(rstd).double().cpu() - o["rstd"]).abs() / o["rstd"]).max().item()
    return em, er


def judge_ln(pb, got):
    """name -> judgement (``judge_rows`` / ``judge_vec``) of every tensor in ``got`` (name -> the
    kernels' result), plus mean / rstd when given."""
    tols = ln_tols(pb.combo)
    res = {}
    for name, t in got.items():
        if name in tols:
            res[name] = judge_rows(t.float().cpu(), pb.oracle[name], pb.yard[name], tols[name])
        elif name in ("dw", "db"):
            res[name] = judge_vec(t, pb.oracle[name], pb.yard[name])
    if "mean" in got:
        km, kr = stat_errors(pb, got["mean"], got["rstd"])
        ym, yr = stat_errors(pb, pb.yard["mean"], pb.yard["rstd"])
        for name, k, y in (("mean", km, ym), ("rstd", kr, yr)):
            res[name] = types.SimpleNamespace(kernel=k, where=None, yardstick=y, bar=TOL[F32], excess=0.0,
                                              over=[] if k < TOL[F32] else [(None, k, TOL[F32])])
    return res


def expected_zero_rows(pb, name):
    """The rows of tensor ``name`` whose oracle must be exactly zero: dx of the zero-dy row
    (unless the fusion adds the stream's gradient there) and xo = x + a of the row of zeros."""
    z = torch.zeros(pb.rows, dtype=torch.bool)
    if pb.plant and name == "dx" and not pb.fused:
        z[pb.plant["zero_dy"]] = True
    if pb.plant and name == "xo":
        z[pb.plant["zeros"]] = True
    return z


# ---- SwiGLU -----------------------------------------------------------------------------------
SWIGLU_TAILS = [0.0, 1e-4, 10.0, 20.0, 87.0, 89.0, 100.0, 1e4]      # and their negatives
# the floor of the element-wise measure: below it a value is under the format's own underflow
# (fp32 / bf16: sigmoid(a) leaves fp32's normal range at a < -87.3, so silu(a) b d is off by up
# to ~1e-36 in absolute terms whatever the algorithm; fp16: one subnormal step, 2^-24, over the
# 2e-2 bar)
SWIGLU_FLOOR = {F32: 1e-30, BF16: 1e-30, F16: 2.0 ** -24 / TOL[F16]}


def swiglu_problem(dtype, rows, n, seed=0, tails=True):
    """a, b, dout as stored in ``dtype`` and the fp64 out, da, db (F.silu(a) * b and autograd),
    plus ``aux``: per output the magnitude that element's error is measured against beyond |ref|
    (da = dout b s (1 + a (1 - s)) cancels near a = -1.28: its terms' size |dout b s|)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + n)
    a = torch.randn(rows, n, generator=g) * 3
    if tails:
        vals = torch.tensor([s * v for v in SWIGLU_TAILS for s in (1.0, -1.0)])
        k = max(1, (rows * n) // 4)
        idx = torch.randperm(rows * n, generator=g)[:k]
        a.view(-1)[idx] = vals[torch.arange(k) % len(vals)]
    a = a.clamp(-torch.finfo(dtype).max, torch.finfo(dtype).max).to(dtype)
    b = torch.randn(rows, n, generator=g).clamp(-4, 4).to(dtype)
    d = torch.randn(rows, n, generator=g).clamp(-4, 4).to(dtype)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    out = F.silu(a64) * b64
    out.backward(d.double())
    sg = torch.sigmoid(a.double())
    aux = {"out": torch.zeros_like(sg), "da": (d.double() * b.double() * sg).abs(), "db": torch.zeros_like(sg)}
    return types.SimpleNamespace(a=a, b=b, d=d, oracle={"out": out.detach(), "da": a64.grad, "db": b64.grad}, aux=aux)


def elem_err(got, ref, aux, dtype):
    """max over elements of |got - ref| / (|ref| + aux + floor)."""
    got, ref = torch.as_tensor(got).double().cpu(), ref.double()
    return ((got - ref).abs() / (ref.abs() + aux + SWIGLU_FLOOR[dtype])).max().item()


# ---- RoPE ---------------------------------------------------------------------------------------
# one rounding of an fp32 result to the destination: at most a unit roundoff of the element (2^-8
# bf16, 2^-11 fp16), so at most that fraction of the row's maximum; the bar is twice it.  fp32: TOL.
ROPE_BAR = {F32: TOL[F32], BF16: 2.0 ** -7, F16: 2.0 ** -10}


def rope_source(B, T, H, N, hs, seed=0):
    """Values every storage dtype holds exactly (multiples of 1/64 up to 4): one fp64 reference
    serves fp32, bf16 and fp16."""
    g = torch.Generator().manual_seed(seed + 131 * T + 17 * H + 7 * N + hs)
    return torch.randint(-256, 257, (B, T, H, N, hs), generator=g).double() / 64


def rope64(x, freqs_c, inverse=False):
    """fp64 rotation of (B, T, H, N, hs) by the complex table's first T rows (its conjugate for
    the inverse), pairs interleaved: test_gpu_parity._rope64 over every (b, h, i)."""
    from test_gpu_parity import _rope64
    B, T, H, N, hs = x.shape
    flat = x.double().permute(0, 2, 3, 1, 4).reshape(B * H * N, T, hs)
    out = _rope64(flat, freqs_c.conj().resolve_conj() if inverse else freqs_c)
    return out.reshape(B, H, N, T, hs).permute(0, 3, 1, 2, 4).contiguous()
