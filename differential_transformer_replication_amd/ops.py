"""torch.autograd.Function wrappers over the C ABI (the only compute path).

``diff_attention(qkv, coef, ...)``
    Fused N-branch causal differential attention over a packed projection
    output ``qkv`` of shape (B, T, W), W = 2*H*N*hs + H*dv, laid out
    ``[Q (H, N, hs) | K (H, N, hs) | V (H, dv)]``.  Returns O of shape
    (B, T, H*dv) = concatenated per-head outputs (diff_transformer.py:89, before
    the GroupLayerNorm).  Backward writes dQ/dK/dV into one (B, T, W) buffer, so
    the projection GEMM's backward sees a single gradient tensor.
``group_ln_scale(x, w, b, eps, out_scale)``
    GroupLayerNorm over the last dim fused with the constant output scale
    (diff_transformer.py:15-20, 90-91).

There is no CPU or eager fallback: non-CUDA tensors raise.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Optional, Tuple

import torch
from torch.nn import functional as F

from . import _lib, packing

Tensor = torch.Tensor


def _require_gpu(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("differential_transformer_replication_amd ops run only on the MI355X "
                               "HIP path (libdiffattn.so); got a tensor on " + str(t.device))


class KernelTimer:
    """Optional HIP-event brackets around the two dominant launches (the fused
    forward kernel and the fused backward kernel).  Events are recorded on the
    stream the kernels are launched on (torch's current stream), so each pair
    brackets exactly one kernel.  Off by default (no events, no overhead)."""

    def __init__(self):
        self.active = False
        self._pairs: Dict[str, List[Tuple[torch.cuda.Event, torch.cuda.Event]]] = {}

    def start(self):
        self._pairs = {}
        self.active = True

    def stop(self):
        self.active = False

    @contextlib.contextmanager
    def region(self, name: str):
        if not self.active:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self._pairs.setdefault(name, []).append((e0, e1))

    def mean_ms(self) -> Dict[str, Tuple[float, int]]:
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v) / len(v), len(v)) for k, v in self._pairs.items()}


TIMER = KernelTimer()


def supported(dtype: torch.dtype, hs: int, N: int, dv: int) -> bool:
    """Whether libdiffattn.so runs this shape as it is (dta_supported): an N-branch
    kernel plan, or branch groups over such plans for branch counts without one."""
    return bool(_lib.load().dta_supported(_lib.dtype_code(dtype), hs, N, dv))


def padded_head(dtype: torch.dtype, hs: int, N: int, dv: int) -> Optional[int]:
    """The head size the kernels run a head of size ``hs`` at: ``hs`` itself when it is
    built, else the smallest built head size above it (Q_i / K_i and V zero-padded, see
    ``diff_attention``), else None.  The reference accepts any head size
    (head_size = n_embd // (2 n_head), diff_transformer.py:111); the plans are built for
    16, 32, 64, 96, 128 and 256 (256: 16-bit diff plans, and the control's dv = hs in every
    dtype)."""
    if N < 1 or hs < 1 or dv not in (hs, 2 * hs) or (dv == hs and N != 1):
        return None
    for hp in (hs,) + tuple(h for h in (16, 32, 64, 96, 128, 256) if h > hs):
        if supported(dtype, hp, N, hp if dv == hs else 2 * hp):
            return hp
    return None


def attention_supported(dtype: torch.dtype, hs: int, N: int, dv: int) -> bool:
    """Whether ``diff_attention`` runs this shape on the HIP kernels (directly or padded)."""
    return padded_head(dtype, hs, N, dv) is not None


def packed_width(H: int, N: int, hs: int, dv: int) -> int:
    return 2 * H * N * hs + H * dv


def split_packed(qkv: Tensor, H: int, N: int, hs: int, dv: int):
    """Strided (B,T,H,N,hs)/(B,T,H,dv) views of the packed projection output."""
    B, T, W = qkv.shape
    nq = H * N * hs
    q = qkv[..., :nq].unflatten(-1, (H, N, hs))
    k = qkv[..., nq:2 * nq].unflatten(-1, (H, N, hs))
    v = qkv[..., 2 * nq:].unflatten(-1, (H, dv))
    return q, k, v


def _obr_dtype(dtype: torch.dtype) -> torch.dtype:
    """Storage type of the saved per-branch outputs O_i (ABI 6 obr_dtype): fp32.  fp16 O_i
    (DTA_OBR_F16=1, 16-bit activations) measured 0.7% off the cfg2 step but left one head's
    d(lambda) at 1.22 relative error in the default-config bf16 model, against a bar of 0.56
    (2x the reference algorithm's own bf16 error; fp32 O_i passes): the cancellation in
    sum_rows delta_i needs O_i unrounded."""
    if dtype != torch.float32 and os.environ.get("DTA_OBR_F16", "0") == "1":
        return torch.float16
    return torch.float32


# Whether the backward hands dta_attn_bwd the fp32 dV workspace (ABI 7 dv_f32) when dK/dV runs
# in more than one branch group.  Always on in the product; the C ABI's other path (dv_f32 NULL:
# each later group adds into the 16-bit dV) is exercised by the GPU tests with it off.
_DV_F32_WORKSPACE = [True]
# Whether the backward hands dta_attn_bwd the ABI 8 lse_c workspace (16-bit, no dropout: the key-major
# kernel folds |c_i| into its probabilities).  Always on in the product; the GPU tests turn it off to
# run the C ABI's unfolded 16-bit path.
_LSE_C_WORKSPACE = [True]

# Backward branch-group caps handed to dta_attn_bwd (ABI 7 group_max_dq / group_max_dkdv);
# (0, 0) = the library's per-stage defaults.  Tests set them with ``bwd_group_caps`` to run
# every built native N-branch backward plan.
_BWD_GROUP_MAX = [0, 0]


@contextlib.contextmanager
def bwd_group_caps(dq: int, dkdv: int):
    """Forward passes run within the block have their backward run dQ in branch groups of
    at most ``dq`` and dK/dV in groups of at most ``dkdv`` (0 = the library default for that
    stage).  The caps are taken at the forward and kept on the autograd context, so the
    backward may run after the block exits."""
    old = list(_BWD_GROUP_MAX)
    _BWD_GROUP_MAX[:] = [int(dq), int(dkdv)]
    try:
        yield
    finally:
        _BWD_GROUP_MAX[:] = old


class _DiffAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv: Tensor, coef: Tensor, H: int, N: int, hs: int, freqs: Optional[Tensor], dv: int,
                dropout_p: float, seed: int, scale: float):
        lib = _lib.load()
        _require_gpu(qkv, coef)
        if qkv.dim() != 3:
            raise RuntimeError("qkv must be (B, T, W)")
        qkv = qkv.contiguous()
        B, T, W = qkv.shape
        if W != packed_width(H, N, hs, dv):
            raise RuntimeError(f"packed width {W} != 2*H*N*hs + H*dv = {packed_width(H, N, hs, dv)}")
        dt = _lib.dtype_code(qkv.dtype)
        if not lib.dta_supported(dt, hs, N, dv):
            raise RuntimeError(f"no gfx950 kernel for head_size={hs}, n_terms={N}, dv={dv}, dtype={qkv.dtype}")
        coef = coef.detach().to(torch.float32).contiguous()
        dev = qkv.device
        stream = _lib.stream_handle(dev)
        q, k, v = split_packed(qkv, H, N, hs, dv)
        qk_rot = None
        rope_args = (None, _lib.DtaTensor())
        if freqs is not None:
            # RoPE of every Q_i/K_i (Ndiff_transformer.py:104-109): the K_i by one rotation pass,
            # the Q_i inside the forward kernel as it loads them (it also stores the rotated
            # rows into qk_rot for the backward)
            qk_rot = torch.empty(B, T, 2 * H, N, hs, device=dev, dtype=qkv.dtype)
            src = k
            ra = _lib.RopeArgs(dt, B, T, H, N, hs, 0, 0, _lib.tensor5(src), _lib.tensor5(qk_rot[:, :, H:]),
                               freqs.data_ptr())
            _lib.check(lib.dta_rope(ra, stream))
            k = qk_rot[:, :, H:]
            rope_args = (freqs.data_ptr(), _lib.tensor5(qk_rot[:, :, :H]))
        o = torch.empty(B, T, H, dv, device=dev, dtype=qkv.dtype)
        # the per-branch O_i for delta_i = <dO, O_i> (hence d(coef), d(lambda)), fp32
        obr = torch.empty(N, B, T, H, dv, device=dev, dtype=_obr_dtype(qkv.dtype))
        lse = torch.empty(N, B, H, T, device=dev, dtype=torch.float32)
        obr_t = _lib.DtaTensor(obr.data_ptr(), *obr.stride()[1:4], obr.stride(0))
        a = _lib.AttnFwdArgs(dt, B, T, H, N, hs, dv, scale, dropout_p,
                             _lib.tensor5(q), _lib.tensor5(k), _lib.tensor5(v), _lib.tensor5(o), obr_t,
                             lse.data_ptr(), coef.data_ptr(), seed, *rope_args, _lib.dtype_code(obr.dtype))
        with TIMER.region("attn_fwd"):
            _lib.check(lib.dta_attn_fwd(a, stream))
        ctx.save_for_backward(qkv, qk_rot, obr, lse, coef, freqs)
        ctx.dims = (H, N, hs, dv, scale)
        ctx.drop = (dropout_p, seed)
        # the backward branch-group caps in force at the forward (bwd_group_caps): saved here, so
        # a backward run after the block exits (or on another thread) uses the same caps
        ctx.caps = tuple(_BWD_GROUP_MAX)
        return o.view(B, T, H * dv)

    @staticmethod
    def backward(ctx, do: Tensor):
        lib = _lib.load()
        qkv, qk_rot, obr, lse, coef, freqs = ctx.saved_tensors
        H, N, hs, dv, scale = ctx.dims
        B, T, W = qkv.shape
        dev = qkv.device
        stream = _lib.stream_handle(dev)
        dt = _lib.dtype_code(qkv.dtype)
        do = do.to(qkv.dtype).contiguous().view(B, T, H, dv)
        q, k, v = split_packed(qkv, H, N, hs, dv)
        if qk_rot is not None:
            q, k = qk_rot[:, :, :H], qk_rot[:, :, H:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dvv = split_packed(dqkv, H, N, hs, dv)
        dcoef = torch.empty(H, N, device=dev, dtype=torch.float32)
        delta = torch.empty(N, B, H, T, device=dev, dtype=torch.float32)
        # d(coef) from per-wave partials summed in a fixed order: reproducible lambda grads
        dcp = torch.empty(lib.dta_attn_bwd_dcoef_partial_bytes(B, T, H, N) // 4, device=dev, dtype=torch.float32)
        # dK/dV in more than one branch group: dV summed in fp32 across the groups (one rounding)
        dv32 = None
        caps = ctx.caps
        if dt != _lib.DTA_F32 and _DV_F32_WORKSPACE[0] and lib.dta_attn_bwd_dkdv_groups(dt, hs, N, dv, caps[1]) > 1:
            dv32 = torch.empty(B, T, H, dv, device=dev, dtype=torch.float32)
        # ABI 8: the |c_i|-folded key-major kernel's score seeds (16-bit, no dropout; private workspace)
        lsec = (torch.empty(N, B, H, T, device=dev, dtype=torch.float32)
                if dt != _lib.DTA_F32 and ctx.drop[0] == 0.0 and _LSE_C_WORKSPACE[0] else None)
        # with RoPE the kernels differentiate w.r.t. the rotated Q/K (qk_rot) and their
        # dQ / dK epilogues apply the inverse rotation, writing straight into dqkv
        obr_t = _lib.DtaTensor(obr.data_ptr(), *obr.stride()[1:4], obr.stride(0))
        a = _lib.AttnBwdArgs(dt, B, T, H, N, hs, dv, scale, ctx.drop[0],
                             _lib.tensor5(q), _lib.tensor5(k), _lib.tensor5(v), obr_t,
                             lse.data_ptr(), coef.data_ptr(), _lib.tensor5(do),
                             _lib.tensor5(dq), _lib.tensor5(dk), _lib.tensor5(dvv),
                             dcoef.data_ptr(), delta.data_ptr(), None, _lib.BWD_PRE,
                             freqs.data_ptr() if freqs is not None else None, dcp.data_ptr(), ctx.drop[1],
                             _lib.dtype_code(obr.dtype), *caps,
                             dv32.data_ptr() if dv32 is not None else None,
                             lsec.data_ptr() if lsec is not None else None)
        # (no PRE stage: with the d(coef) partials the DQ stage's ordered reduce writes dcoef whole)
        a.stages = _lib.BWD_DQ
        with TIMER.region("attn_bwd_dq"):
            _lib.check(lib.dta_attn_bwd(a, stream))
        a.stages = _lib.BWD_DKDV
        with TIMER.region("attn_bwd_dkdv"):
            _lib.check(lib.dta_attn_bwd(a, stream))
        return dqkv, dcoef, None, None, None, None, None, None, None, None


def diff_attention(qkv: Tensor, coef: Tensor, H: int, N: int, hs: int,
                   freqs: Optional[Tensor] = None, dv: Optional[int] = None, dropout_p: float = 0.0,
                   seed: Optional[int] = None) -> Tensor:
    """O = sum_i coef[h,i] dropout(softmax_causal(Q_i K_i^T/sqrt(hs))) V for every head.

    ``freqs``: fp32 (T, hs/2, 2) rotary table (view_as_real of freqs_cis[:T]) or None.
    ``dv``: value width per head; 2*hs for the differential models (default), hs for
    standard attention (N=1, coef 1: control.py:38-63).
    ``dropout_p``: nn.Dropout on every attention map (diff_transformer.py:66-67): each
    map element kept with probability 1-p and scaled by 1/(1-p), independently per map,
    from a counter-based hash of ``seed`` (include/diffattn.h); by default the seed is
    drawn from torch's generator, so ``torch.manual_seed`` makes runs repeatable.
    """
    if freqs is not None:
        freqs = freqs.to(device=qkv.device, dtype=torch.float32).contiguous()
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), got {dropout_p}")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if dropout_p > 0 else 0
    dv = 2 * hs if dv is None else dv
    scale = 1.0 / math.sqrt(hs)                 # diff_transformer.py:57, of the true head size
    hp = padded_head(qkv.dtype, hs, N, dv) if qkv.is_cuda else hs
    if hp is None:
        raise RuntimeError(f"no gfx950 kernel for head_size={hs}, n_terms={N}, dv={dv}, dtype={qkv.dtype} "
                           "(head sizes up to 256 are served; 129-256 in 16-bit for the differential models)")
    if hp == hs:
        return _DiffAttention.apply(qkv, coef, H, N, hs, freqs, dv, dropout_p, int(seed), scale)
    # a head size without its own plan runs in the next built one: Q_i / K_i zero-padded
    # to hp columns leave every score Q_i K_i^T unchanged (the softmax scale stays
    # 1/sqrt(hs)), V padded to dvp columns adds zero output columns, which are dropped;
    # the pad columns' gradients are discarded by the slices' backward
    dvp = hp if dv == hs else 2 * hp
    B, T, _ = qkv.shape
    q, k, v = split_packed(qkv, H, N, hs, dv)
    qkv_p = torch.cat([F.pad(q, (0, hp - hs)).flatten(2), F.pad(k, (0, hp - hs)).flatten(2),
                       F.pad(v, (0, dvp - dv)).flatten(2)], dim=-1)
    if freqs is not None:
        # identity rotation (cos 1, sin 0) on the pad pairs: they stay zero
        pad = torch.zeros(freqs.shape[0], (hp - hs) // 2, 2, device=freqs.device, dtype=freqs.dtype)
        pad[..., 0] = 1.0
        freqs = torch.cat([freqs, pad], dim=1).contiguous()
    out = _DiffAttention.apply(qkv_p, coef, H, N, hp, freqs, dvp, dropout_p, int(seed), scale)
    return out.view(B, T, H, dvp)[..., :dv].reshape(B, T, H * dv)


class _GroupLNScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Tensor, eps: float, out_scale: float, holder=None,
                y_dtype: Optional[torch.dtype] = None):
        lib = _lib.load()
        _require_gpu(x, w, b)
        # bound (dp.BucketedAllReduce, packing.bind_grad): dw/db accumulate straight into
        # the parameters' bucket-view gradients -- no zeros, no AccumulateGrad adds
        ctx.bound = (holder, (w, b)) if holder is not None and "grad" in holder else None
        C = x.shape[-1]
        x2 = x.contiguous().view(-1, C)
        rows = x2.shape[0]
        w32 = w.detach().to(torch.float32).contiguous().view(-1)
        b32 = b.detach().to(torch.float32).contiguous().view(-1)
        if w32.numel() != C or b32.numel() != C:
            raise RuntimeError("GroupLayerNorm weight/bias size must equal the normalised width")
        # io: an fp32 input normalised straight into a 16-bit output (and its backward
        # from that dtype's gradient), dta_ln_args.io_dtype
        io = 0
        if y_dtype is not None and y_dtype != x.dtype:
            if x.dtype != torch.float32 or y_dtype not in (torch.bfloat16, torch.float16):
                raise RuntimeError("LayerNorm output dtype may differ only for fp32 input and 16-bit output")
            io = 1 + _lib.dtype_code(y_dtype)
        y = torch.empty(x2.shape, device=x.device, dtype=y_dtype if io else x.dtype)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        a = _lib.LnArgs(_lib.dtype_code(x.dtype), rows, C, eps, out_scale, x2.data_ptr(), C, y.data_ptr(), C,
                        w32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, 0, None, 0,
                        None, None, None, io)
        ctx.io = (io, y.dtype)
        _lib.check(lib.dta_ln_fwd(a, _lib.stream_handle(x.device)))
        ctx.save_for_backward(x2, w32, mean, rstd)
        ctx.meta = (eps, out_scale, x.shape, w.dtype, w.shape, b.dtype, b.shape)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy: Tensor):
        lib = _lib.load()
        x2, w32, mean, rstd = ctx.saved_tensors
        eps, out_scale, xshape, wdt, wshape, bdt, bshape = ctx.meta
        C = x2.shape[1]
        io, ydt = ctx.io
        dy2 = dy.to(ydt).contiguous().view(-1, C)
        dx = torch.empty_like(x2)
        g = None
        if ctx.bound is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            holder, params = ctx.bound
            g = packing._grad_target(holder, params)
            if g is not None and g.numel() != 2 * C:
                g = None
        if g is not None:
            dw, db = g[:C], g[C:]
        else:
            dw = torch.zeros(C, device=x2.device, dtype=torch.float32)
            db = torch.zeros(C, device=x2.device, dtype=torch.float32)
        # per-block column partials summed in order: reproducible dw / db (no atomics)
        part = torch.empty(lib.dta_ln_bwd_workspace_bytes(x2.shape[0], C) // 4, device=x2.device, dtype=torch.float32)
        a = _lib.LnArgs(_lib.dtype_code(x2.dtype), x2.shape[0], C, eps, out_scale, x2.data_ptr(), C, None, 0,
                        w32.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(), dy2.data_ptr(), C,
                        dx.data_ptr(), C, dw.data_ptr(), db.data_ptr(), part.data_ptr(), io)
        _lib.check(lib.dta_ln_bwd(a, _lib.stream_handle(x2.device)))
        if g is not None:
            hook = ctx.bound[0]["on_ready"]
            for p in ctx.bound[1]:
                hook(p)
            return dx.view(xshape), None, None, None, None, None, None
        return dx.view(xshape), dw.to(wdt).view(wshape), db.to(bdt).view(bshape), None, None, None, None


class _AddLN(torch.autograd.Function):
    """(x + a, LayerNorm(x + a)) in one pass: a Block's residual add feeding its next
    pre-LN (diff_transformer.py:121-125), fp32 residual stream x, 16-bit branch output a
    and LN output.  Backward: the residual gradient d(x + a) plus the LN backward, in one
    pass that also writes the branch's 16-bit gradient."""

    @staticmethod
    def forward(ctx, x: Tensor, a: Tensor, w: Tensor, b: Tensor, eps: float, holder, ydt: torch.dtype):
        lib = _lib.load()
        _require_gpu(x, a, w, b)
        C = x.shape[-1]
        x2 = x.contiguous().view(-1, C)
        a2 = a.to(ydt).contiguous().view(-1, C)
        rows = x2.shape[0]
        w32 = w.detach().to(torch.float32).contiguous().view(-1)
        b32 = b.detach().to(torch.float32).contiguous().view(-1)
        xo = torch.empty_like(x2)
        y = torch.empty(x2.shape, device=x.device, dtype=ydt)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        io = 1 + _lib.dtype_code(ydt)
        args = _lib.LnArgs(_lib.DTA_F32, rows, C, eps, 1.0, x2.data_ptr(), C, y.data_ptr(), C,
                           w32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, 0, None, 0,
                           None, None, None, io, a2.data_ptr(), C, xo.data_ptr(), C)
        _lib.check(lib.dta_ln_fwd(args, _lib.stream_handle(x.device)))
        ctx.bound = (holder, (w, b)) if holder is not None and "grad" in holder else None
        ctx.save_for_backward(xo, w32, mean, rstd)
        ctx.meta = (eps, x.shape, a.dtype, ydt, w.dtype, w.shape, b.dtype, b.shape, io)
        return xo.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, dxo: Optional[Tensor], dy: Optional[Tensor]):
        lib = _lib.load()
        xo, w32, mean, rstd = ctx.saved_tensors
        eps, xshape, adt, ydt, wdt, wshape, bdt, bshape, io = ctx.meta
        C = xo.shape[1]
        dy2 = (dy.to(ydt).contiguous().view(-1, C) if dy is not None
               else torch.zeros(xo.shape, device=xo.device, dtype=ydt))
        dres = dxo.to(torch.float32).contiguous().view(-1, C) if dxo is not None else None
        dx = torch.empty_like(xo)
        da = torch.empty(xo.shape, device=xo.device, dtype=ydt)
        g = None
        if ctx.bound is not None and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]:
            holder, params = ctx.bound
            g = packing._grad_target(holder, params)
            if g is not None and g.numel() != 2 * C:
                g = None
        if g is not None:
            dw, db = g[:C], g[C:]
        else:
            dw = torch.zeros(C, device=xo.device, dtype=torch.float32)
            db = torch.zeros(C, device=xo.device, dtype=torch.float32)
        part = torch.empty(lib.dta_ln_bwd_workspace_bytes(xo.shape[0], C) // 4, device=xo.device, dtype=torch.float32)
        args = _lib.LnArgs(_lib.DTA_F32, xo.shape[0], C, eps, 1.0, xo.data_ptr(), C, None, 0, w32.data_ptr(), None,
                           mean.data_ptr(), rstd.data_ptr(), dy2.data_ptr(), C, dx.data_ptr(), C, dw.data_ptr(),
                           db.data_ptr(), part.data_ptr(), io, None, 0, None, 0,
                           dres.data_ptr() if dres is not None else None, C, da.data_ptr(), C)
        _lib.check(lib.dta_ln_bwd(args, _lib.stream_handle(xo.device)))
        da_out = da.view(xshape).to(adt)
        if g is not None:
            hook = ctx.bound[0]["on_ready"]
            for p in ctx.bound[1]:
                hook(p)
            return dx.view(xshape), da_out, None, None, None, None, None
        return dx.view(xshape), da_out, dw.to(wdt).view(wshape), db.to(bdt).view(bshape), None, None, None


def add_layer_norm(x: Tensor, a: Tensor, ln: "LayerNorm"):
    """(x + a, ln(x + a)) -- a Block's residual add and the following pre-LN
    (diff_transformer.py:121-125).  One fused pass when x is the fp32 residual stream
    under autocast and ln emits the autocast dtype; otherwise the two ops."""
    C = x.shape[-1]
    if (x.is_cuda and x.dtype == torch.float32 and isinstance(ln, LayerNorm) and ln.autocast_out
            and torch.is_autocast_enabled("cuda") and ln.weight is not None and ln.bias is not None
            and len(ln.normalized_shape) == 1 and C % 8 == 0 and C <= 8192 and a.shape == x.shape
            and a.dtype in (torch.bfloat16, torch.float16)):
        ydt = torch.get_autocast_dtype("cuda")
        with torch.autocast("cuda", enabled=False):
            return _AddLN.apply(x, a, ln.weight, ln.bias, ln.eps, ln._gpack, ydt)
    xo = x + a
    return xo, ln(xo)


def group_ln_scale(x: Tensor, w: Tensor, b: Tensor, eps: float = 1e-5, out_scale: float = 1.0,
                   holder: Optional[Dict] = None) -> Tensor:
    """``holder``: the module's grad-binding dict (``param_packs``), or None."""
    return _GroupLNScale.apply(x, w, b, eps, out_scale, holder, None)


class LayerNorm(torch.nn.LayerNorm):
    """``nn.LayerNorm`` of the Blocks (``ln1``/``ln2``/``ln_f``: diff_transformer.py:111-126,
    Ndiff_transformer.py:164-179, control.py:92-111) on the HIP LN kernels for GPU
    tensors: same parameters, ``state_dict`` keys and fp32 statistics; under autocast
    it normalises in fp32 like ``F.layer_norm``'s autocast rule.  Host tensors (the
    control model on the CPU) and shapes the kernels do not take keep PyTorch's."""

    def __init__(self, *args, autocast_out: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self._gpack = {}                      # grad binding of (weight, bias), dp.BucketedAllReduce
        # autocast_out: under autocast, write the output in the autocast dtype -- exact
        # when every consumer is an autocast GEMM (which would cast it anyway: the
        # Blocks' ln1/ln2/ln_f), and it saves the separate cast there and back
        self.autocast_out = autocast_out

    def param_packs(self):
        return [(self._gpack, [self.weight, self.bias])] if self.weight is not None and self.bias is not None else []

    def forward(self, x: Tensor) -> Tensor:
        C = x.shape[-1]
        if (not x.is_cuda or len(self.normalized_shape) != 1 or self.weight is None or self.bias is None
                or C % 8 or C > 8192):
            return super().forward(x)
        ydt = None
        if torch.is_autocast_enabled("cuda"):
            if x.dtype != torch.float32:
                x = x.float()
            if self.autocast_out:
                ydt = torch.get_autocast_dtype("cuda")
        with torch.autocast("cuda", enabled=False):
            return _GroupLNScale.apply(x, self.weight, self.bias, self.eps, 1.0, self._gpack, ydt)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        lib = _lib.load()
        _require_gpu(a, b)
        if a.shape != b.shape:
            raise RuntimeError("SwiGLU branches must have one shape")
        dt = torch.promote_types(a.dtype, b.dtype)
        a2 = a.to(dt).contiguous().view(-1, a.shape[-1])
        b2 = b.to(dt).contiguous().view(-1, a.shape[-1])
        out = torch.empty_like(a2)
        n = a2.shape[1]
        sa = _lib.SwigluArgs(_lib.dtype_code(dt), a2.shape[0], n, a2.data_ptr(), n, b2.data_ptr(), n,
                             out.data_ptr(), n, None, 0, None, 0, None, 0)
        _lib.check(lib.dta_swiglu_fwd(sa, _lib.stream_handle(a.device)))
        ctx.save_for_backward(a2, b2)
        ctx.meta = (a.shape, a.dtype, b.dtype)
        return out.view(a.shape)

    @staticmethod
    def backward(ctx, dout: Tensor):
        lib = _lib.load()
        a2, b2 = ctx.saved_tensors
        shape, adt, bdt = ctx.meta
        n = a2.shape[1]
        d2 = dout.to(a2.dtype).contiguous().view(-1, n)
        da, db = torch.empty_like(a2), torch.empty_like(b2)
        sa = _lib.SwigluArgs(_lib.dtype_code(a2.dtype), a2.shape[0], n, a2.data_ptr(), n, b2.data_ptr(), n,
                             None, 0, d2.data_ptr(), n, da.data_ptr(), n, db.data_ptr(), n)
        _lib.check(lib.dta_swiglu_bwd(sa, _lib.stream_handle(a2.device)))
        return da.view(shape).to(adt), db.view(shape).to(bdt)


def swiglu(a: Tensor, b: Tensor) -> Tensor:
    """``F.silu(a) * b`` in one pass forward and one backward (SwiGLU.forward of the
    reference models); GPU tensors whose last dim is a multiple of 8."""
    if not a.is_cuda or a.shape[-1] % 8 or a.shape != b.shape:
        return F.silu(a) * b
    return _SwiGLU.apply(a, b)


def _swiglu_launch(y2: Tensor, n: int, out: Optional[Tensor], dout: Optional[Tensor], dy: Optional[Tensor],
                   dbias: Optional[Tensor] = None):
    """dta_swiglu over the column halves of a packed (rows, 2n) projection: a = y2[:, :n],
    b = y2[:, n:]; forward writes ``out`` (rows, n), backward writes da | db into the halves
    of ``dy`` (rows, 2n)."""
    lib = _lib.load()
    es, rows, w = y2.element_size(), y2.shape[0], 2 * n
    a, b = y2.data_ptr(), y2.data_ptr() + n * es
    if dy is None:
        sa = _lib.SwigluArgs(_lib.dtype_code(y2.dtype), rows, n, a, w, b, w, out.data_ptr(), n,
                             None, 0, None, 0, None, 0)
        _lib.check(lib.dta_swiglu_fwd(sa, _lib.stream_handle(y2.device)))
    else:
        work = None
        if dbias is not None:
            work = torch.empty(lib.dta_swiglu_bwd_workspace_bytes(rows, n) // 4 + 4, device=y2.device,
                               dtype=torch.float32)
        sa = _lib.SwigluArgs(_lib.dtype_code(y2.dtype), rows, n, a, w, b, w, None, 0, dout.data_ptr(), n,
                             dy.data_ptr(), w, dy.data_ptr() + n * es, w,
                             dbias.data_ptr() if dbias is not None else None,
                             work.data_ptr() if work is not None else None)
        _lib.check(lib.dta_swiglu_bwd(sa, _lib.stream_handle(y2.device)))


class _PackedSwiGLU(torch.autograd.Function):
    """SwiGLU with its gate and xform Linears as ONE GEMM over a shared weight pack
    ``[W_gate; W_xform]`` (and bias pack): one (rows, 2n) projection whose halves feed
    the fused SwiGLU kernel; backward writes dA | dB into one (rows, 2n) gradient, so
    dX is one GEMM (K = 2n) instead of two plus an add, dW one GEMM and the bias
    gradient one column sum.  Casts as autocast applies them to the two nn.Linear."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, wbase, bbase, wholder, bholder, *params):
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else x.dtype
        xc = x.to(dt)
        wc, bc = wbase.to(dt), bbase.view(-1).to(dt)
        with torch.autocast("cuda", enabled=False):
            y = F.linear(xc, wc, bc)
        n = wc.shape[0] // 2
        y2 = y.view(-1, 2 * n)
        out = torch.empty(y2.shape[0], n, device=y.device, dtype=y.dtype)
        _swiglu_launch(y2, n, out, None, None)
        ctx.save_for_backward(xc, wc, y2)
        ctx.x_dtype, ctx.w_dtype, ctx.n = x.dtype, wbase.dtype, n
        ctx.wrows = [params[0].shape[0], params[1].shape[0]]
        bound = (wholder is not None and "grad" in wholder and bholder is not None and "grad" in bholder)
        ctx.holders = (wholder, bholder) if bound else None
        ctx.params = params if bound else None
        return out.view(*x.shape[:-1], n)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        xc, wc, y2 = ctx.saved_tensors
        n = ctx.n
        d2 = dout.to(y2.dtype).contiguous().view(-1, n)
        dy = torch.empty_like(y2)
        # the bias gradient (column sums of dA | dB as stored) comes out of the same pass
        db = torch.empty(2 * n, device=y2.device, dtype=torch.float32)
        _swiglu_launch(y2, n, None, d2, dy, db)
        with torch.autocast("cuda", enabled=False):
            dx = (dy @ wc).view(*xc.shape[:-1], xc.shape[-1]).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            dw = packing.weight_grad(dy, xc.reshape(-1, xc.shape[-1]))
        if ctx.holders is not None and all(ctx.needs_input_grad[5:]):
            wh, bh = ctx.holders
            gw = packing._grad_target(wh, ctx.params[:2])
            gb = packing._grad_target(bh, ctx.params[2:])
            if gw is not None and gb is not None:
                packing.accumulate(gw, dw)          # one launch each, bf16 -> fp32 in the add
                packing.accumulate(gb, db)
                for h, ps in ((wh, ctx.params[:2]), (bh, ctx.params[2:])):
                    for p in ps:
                        h["on_ready"](p)
                return (dx, None, None, None, None) + (None,) * 4
        dw = dw.to(ctx.w_dtype)
        db = db.to(ctx.w_dtype)
        gwg, gwx = torch.split(dw, ctx.wrows, 0)
        gbg, gbx = torch.split(db, ctx.wrows, 0)
        return (dx, None, None, None, None, gwg, gwx, gbg, gbx)


class _Linear(torch.autograd.Function):
    """``nn.Linear`` under the same autocast casts, with its weight gradient through
    ``packing.weight_grad`` (fp32 output, split over tokens when the output is small)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, w, b):
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else x.dtype
        xc, wc = x.to(dt), w.to(dt)
        bc = b.to(dt) if b is not None else None
        with torch.autocast("cuda", enabled=False):
            y = F.linear(xc, wc, bc)
        ctx.save_for_backward(xc, wc)
        ctx.dtypes = (x.dtype, w.dtype, b.dtype if b is not None else None)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        xdt, wdt, bdt = ctx.dtypes
        dy2 = dy.to(wc.dtype).reshape(-1, wc.shape[0])
        with torch.autocast("cuda", enabled=False):
            dx = (dy2 @ wc).view(*xc.shape[:-1], wc.shape[1]).to(xdt) if ctx.needs_input_grad[0] else None
            dw = packing.weight_grad(dy2, xc.reshape(-1, xc.shape[-1])).to(wdt) if ctx.needs_input_grad[1] else None
            db = dy2.sum(0).to(bdt) if bdt is not None and ctx.needs_input_grad[2] else None
        return dx, dw, db


def linear(x: Tensor, mod: torch.nn.Linear) -> Tensor:
    """``mod(x)`` for the reference's nn.Linear layers on the hot path's callers (the MHA
    output projection, the FFN output); GPU: ``_Linear``, else the module itself."""
    if not x.is_cuda or not x.is_floating_point():
        return mod(x)
    return _Linear.apply(x, mod.weight, mod.bias)


def ffn(seq: torch.nn.Sequential, x: Tensor) -> Tensor:
    """The Block's ``ffwd = Sequential(SwiGLU, Linear(4C, C), Dropout)`` (diff_transformer.py:114-119)
    with its Linear through ``linear``."""
    return seq[2](linear(seq[0](x), seq[1]))


def packed_swiglu(x: Tensor, gate: torch.nn.Linear, xform: torch.nn.Linear, wholder: Dict, bholder: Dict) -> Tensor:
    """SwiGLU.forward of the reference models (silu(W_g x + b_g) * (W_x x + b_x)) with
    both Linears' parameters as row views of shared packs (packing.ensure_packed)."""
    wparams, bparams = [gate.weight, xform.weight], [gate.bias, xform.bias]
    n = gate.weight.shape[0]
    if (not x.is_cuda or n % 8 or xform.weight.shape != gate.weight.shape or gate.bias is None
            or xform.bias is None or gate.weight.dtype != xform.weight.dtype):
        return swiglu(gate(x), xform(x))
    wbase = packing.ensure_packed(wparams, wholder)
    bbase = packing.ensure_packed(bparams, bholder)
    return _PackedSwiGLU.apply(x, wbase, bbase, wholder, bholder, *wparams, *bparams)


# ------------------------------------------------------------------ decode ---
def rope_rows(src: Tensor, dst: Tensor, table: Tensor) -> None:
    """dst = RoPE(src) for (B, T, H, N, hs) views whose rows are the positions of
    ``table`` (fp32 (T, hs/2, 2), already sliced to those positions).  No autograd:
    the KV-cache path of generate() only (Ndiff_transformer.py:11-22, 104-109)."""
    lib = _lib.load()
    _require_gpu(src, dst, table)
    B, T, H, N, hs = src.shape
    table = table.to(device=src.device, dtype=torch.float32).contiguous()
    ra = _lib.RopeArgs(_lib.dtype_code(dst.dtype), B, T, H, N, hs, 0, 0, _lib.tensor5(src), _lib.tensor5(dst),
                       table.data_ptr())
    _lib.check(lib.dta_rope(ra, _lib.stream_handle(src.device)))


def _decode(lib, q: Tensor, k: Tensor, v: Tensor, coef: Tensor, bound: int, T_cap: int,
            length_dev: Optional[Tensor] = None, lengths: Optional[Tensor] = None, page=None,
            scale_pool: Optional[Tensor] = None, plan=None) -> Tensor:
    """The launch every decode op ends in, on views its caller has checked.  ``bound``: the host
    length (upper bound), which sizes the grid.  ``lengths`` None: ``dta_attn_decode`` with its
    optional device scalar ``length_dev``; else the ragged entry point, with ``page`` =
    (block_table, P, max_pages, n_pages) the paged one and with ``scale_pool`` the fp8 one;
    ``plan`` (a ``SharedDecodePlan``): the paged entry points' shared-prefix twins."""
    B, H, N, hs = q.shape
    dv = v.shape[-1]
    coef = coef.detach().to(torch.float32).contiguous()
    o = torch.empty(B, 1, H, dv, device=q.device, dtype=q.dtype)
    nbytes = lib.dta_attn_decode_workspace_bytes(B, H, N, hs, dv, T_cap)
    ws = torch.empty(nbytes // 4, device=q.device, dtype=torch.float32)
    head = (_lib.dtype_code(q.dtype), B, H, N, hs, dv, bound, T_cap, 1.0 / math.sqrt(hs),
            _lib.tensor5(q.unsqueeze(1)), _lib.tensor5(k), _lib.tensor5(v), _lib.tensor5(o),
            coef.data_ptr(), ws.data_ptr())
    stream = _lib.stream_handle(q.device)
    if lengths is None:
        rc = lib.dta_attn_decode(_lib.DecodeArgs(*head, _lib.ptr(length_dev)), stream)
    elif page is None:
        rc = lib.dta_attn_decode_ragged(_lib.DecodeRaggedArgs(*head, lengths.data_ptr()), stream)
    else:
        table, P, max_pages, n_pages = page
        tail = (lengths.data_ptr(), P, max_pages, n_pages, table.data_ptr())
        if plan is not None:
            groups = (plan.n_groups, _lib.ptr(plan.members), _lib.ptr(plan.rows))
            if scale_pool is None:
                rc = lib.dta_attn_decode_paged_shared(_lib.DecodePagedSharedArgs(*head, *tail, *groups), stream)
            else:
                rc = lib.dta_attn_decode_paged_shared_fp8(_lib.DecodePagedSharedFp8Args(
                    *head, *tail, scale_pool.data_ptr(), scale_pool.stride(0), *groups), stream)
        elif scale_pool is None:
            rc = lib.dta_attn_decode_paged(_lib.DecodePagedArgs(*head, *tail), stream)
        else:
            rc = lib.dta_attn_decode_paged_fp8(
                _lib.DecodePagedFp8Args(*head, *tail, scale_pool.data_ptr(), scale_pool.stride(0)), stream)
    _lib.check(rc)
    return o.view(B, H * dv)


def _cache_shapes(q: Tensor, k_cache: Tensor, v_cache: Tensor) -> int:
    """Shapes of contiguous cache views against q (B, [Tq,] H, N, hs); returns T_cap."""
    B, (H, N, hs) = q.shape[0], q.shape[-3:]
    T_cap, dv = k_cache.shape[1], v_cache.shape[-1]
    if tuple(k_cache.shape) != (B, T_cap, H, N, hs) or tuple(v_cache.shape) != (B, T_cap, H, dv):
        raise RuntimeError("k_cache/v_cache shapes do not match q")
    return T_cap


def _cache_dtype(q: Tensor, k_cache: Tensor, v_cache: Tensor) -> None:
    if q.dtype != k_cache.dtype or q.dtype != v_cache.dtype:
        raise RuntimeError("q, k_cache and v_cache must share a dtype")


def _coef_shape(coef: Tensor, H: int, N: int) -> None:
    if tuple(coef.shape) != (H, N):
        raise RuntimeError(f"coef must be (H, N) = ({H}, {N})")


def _batch_int32(t: Tensor, B: int, like: Tensor, name: str) -> None:
    if not isinstance(t, Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != like.device:
        raise RuntimeError(f"{name} must be a device int32 tensor of shape ({B},) on {like.device}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _decode_bound(max_length: Optional[int], T_cap: int) -> int:
    """The host upper bound of every length of a ragged decode; default T_cap."""
    max_length = T_cap if max_length is None else int(max_length)
    if not 1 <= max_length <= T_cap:
        raise RuntimeError(f"decode max_length {max_length} outside [1, {T_cap}]")
    return max_length


def _step_operands(q: Tensor, coef: Tensor, pos: Tensor, counts: Optional[Tensor], T_cap: int, owner: str) -> None:
    """coef, pos / counts and Tq of a ragged multi-row step against the ``owner``'s (cache's, table's) T_cap."""
    B, Tq, H, N, _ = q.shape
    _coef_shape(coef, H, N)
    _batch_int32(pos, B, q, "pos")
    if counts is not None:
        _batch_int32(counts, B, q, "counts")
    if Tq > T_cap:
        raise RuntimeError(f"{Tq} new rows do not fit the {owner}'s {T_cap} rows")


def diff_attention_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, coef: Tensor, length: int,
                          length_dev: Optional[Tensor] = None) -> Tensor:
    """One new query row per (b, h) against the first ``length`` cached keys:
    o = sum_i coef[h,i] softmax(q_i K_i[:length]^T / sqrt(hs)) V[:length].

    q: (B, H, N, hs); k_cache: (B, T_cap, H, N, hs); v_cache: (B, T_cap, H, dv)
    (strided views, innermost dim contiguous).  Returns (B, H*dv).  Equals the last
    row of ``diff_attention`` over the same ``length`` positions (the causal mask
    keeps every key up to the query's own position).

    ``length_dev``: optional device int32 scalar holding the length, read by the
    kernels, so one captured HIP graph serves every position; ``length`` is then
    its upper bound (the cache capacity)."""
    lib = _lib.load()
    _require_gpu(q, k_cache, v_cache, coef)
    B, H, N, hs = q.shape
    T_cap = _cache_shapes(q, k_cache, v_cache)
    if not 1 <= length <= T_cap:
        raise RuntimeError(f"decode length {length} outside [1, {T_cap}]")
    _cache_dtype(q, k_cache, v_cache)
    if length_dev is not None:
        _require_gpu(length_dev)
        if length_dev.dtype != torch.int32 or length_dev.numel() != 1:
            raise RuntimeError("length_dev must be one device int32")
    return _decode(lib, q, k_cache, v_cache, coef, length, T_cap, length_dev=length_dev)


# ------------------------------------------------------------------ extend ---
def extend_supported(dtype: torch.dtype, hs: int, N: int, dv: int) -> bool:
    """Whether ``diff_attention_extend`` has a kernel plan for this shape
    (dta_extend_supported): hs % 16 == 0 in 16..128, dv % 32 == 0 up to 256, N <= 8."""
    return bool(_lib.load().dta_extend_supported(_lib.dtype_code(dtype), hs, N, dv))


def _extend(lib, q: Tensor, k: Tensor, v: Tensor, coef: Tensor, T_cap: int, pos: Optional[int] = None,
            pos_dev: Optional[Tensor] = None, counts: Optional[Tensor] = None, page=None,
            scale_pool: Optional[Tensor] = None, rows: bool = False) -> Tensor:
    """The tail every extend op ends in, on views its caller has checked: the kernel-plan check
    (no fallback), then the launch.  ``pos``: the host position of ``dta_attn_extend``;
    ``pos_dev`` / ``counts``: the ragged entry point's, with ``page`` = (block_table, P,
    max_pages, n_pages) the paged one's and with ``scale_pool`` the fp8 one's.  ``rows``: the
    same step on the split-key decode plan (``dta_attn_decode_rows*``, ragged forms only)."""
    B, Tq, H, N, hs = q.shape
    dv = v.shape[-1]
    if rows:
        return _decode_rows(lib, q, k, v, coef, T_cap, pos_dev, counts, page, scale_pool)
    if not (extend_supported if scale_pool is None else extend_fp8_supported)(q.dtype, hs, N, dv):
        raise RuntimeError(f"no extend kernel plan for head_size {hs}, n_terms {N}, dv {dv}, {q.dtype}"
                           + ("" if scale_pool is None else " on an fp8 pool"))
    coef = coef.detach().to(torch.float32).contiguous()
    o = torch.empty(B, Tq, H, dv, device=q.device, dtype=q.dtype)
    if B * Tq == 0:
        return o.view(B, Tq, H * dv)
    head = (_lib.dtype_code(q.dtype), B, H, N, hs, dv, Tq)
    mid = (T_cap, 1.0 / math.sqrt(hs), _lib.tensor5(q), _lib.tensor5(k), _lib.tensor5(v), _lib.tensor5(o),
           coef.data_ptr())
    stream = _lib.stream_handle(q.device)
    if pos_dev is None:
        rc = lib.dta_attn_extend(_lib.ExtendArgs(*head, pos, *mid), stream)
    elif page is None:
        rc = lib.dta_attn_extend_ragged(_lib.ExtendRaggedArgs(*head, *mid, pos_dev.data_ptr(), _lib.ptr(counts)),
                                        stream)
    else:
        table, P, max_pages, n_pages = page
        tail = (pos_dev.data_ptr(), _lib.ptr(counts), P, max_pages, n_pages, table.data_ptr())
        if scale_pool is None:
            rc = lib.dta_attn_extend_paged(_lib.ExtendPagedArgs(*head, *mid, *tail), stream)
        else:
            rc = lib.dta_attn_extend_paged_fp8(
                _lib.ExtendPagedFp8Args(*head, *mid, *tail, scale_pool.data_ptr(), scale_pool.stride(0)), stream)
    _lib.check(rc)
    return o.view(B, Tq, H * dv)


def _decode_rows(lib, q: Tensor, k: Tensor, v: Tensor, coef: Tensor, T_cap: int, pos_dev: Tensor,
                 counts: Optional[Tensor], page, scale_pool: Optional[Tensor]) -> Tensor:
    """``_extend``'s launch on the split-key decode plan: the plan check (no fallback), the
    workspace, then ``dta_attn_decode_rows`` / ``_paged`` / ``_paged_fp8``."""
    B, Tq, H, N, hs = q.shape
    dv = v.shape[-1]
    if not _lib.rows_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no multi-row decode entry points (decode_rows_supported)")
    if not 1 <= Tq <= DECODE_ROWS_MAX:
        raise RuntimeError(f"the multi-row decode takes 1 .. {DECODE_ROWS_MAX} rows per sequence, got {Tq}")
    if not decode_rows_supported(q.dtype, hs, N, dv, Tq, fp8=scale_pool is not None):
        raise RuntimeError(f"no multi-row decode plan for head_size {hs}, n_terms {N}, dv {dv}, {q.dtype}")
    coef = coef.detach().to(torch.float32).contiguous()
    o = torch.empty(B, Tq, H, dv, device=q.device, dtype=q.dtype)
    if B * H == 0:
        return o.view(B, Tq, H * dv)
    nbytes = lib.dta_attn_decode_rows_workspace_bytes(B, H, N, hs, dv, T_cap, Tq)
    ws = torch.empty(nbytes // 4, device=q.device, dtype=torch.float32)
    head = (_lib.dtype_code(q.dtype), B, H, N, hs, dv, Tq, T_cap, 1.0 / math.sqrt(hs),
            _lib.tensor5(q), _lib.tensor5(k), _lib.tensor5(v), _lib.tensor5(o),
            coef.data_ptr(), ws.data_ptr(), pos_dev.data_ptr(), _lib.ptr(counts))
    stream = _lib.stream_handle(q.device)
    if page is None:
        rc = lib.dta_attn_decode_rows(_lib.DecodeRowsArgs(*head), stream)
    else:
        table, P, max_pages, n_pages = page
        tail = (P, max_pages, n_pages, table.data_ptr())
        if scale_pool is None:
            rc = lib.dta_attn_decode_rows_paged(_lib.DecodeRowsPagedArgs(*head, *tail), stream)
        else:
            rc = lib.dta_attn_decode_rows_paged_fp8(
                _lib.DecodeRowsPagedFp8Args(*head, *tail, scale_pool.data_ptr(), scale_pool.stride(0)), stream)
    _lib.check(rc)
    return o.view(B, Tq, H * dv)


def diff_attention_extend(q: Tensor, k_cache: Tensor, v_cache: Tensor, coef: Tensor, pos: int) -> Tensor:
    """``Tq`` new query rows at absolute positions ``pos .. pos+Tq-1`` against the
    cache rows ``0 .. pos+Tq-1`` (the new rows' own K_i / V already written there):
    o[b, r] = sum_i coef[h,i] softmax_j(q_i[b,r] K_i[b,j]^T / sqrt(hs), j <= pos + r) V[b,j].

    q: (B, Tq, H, N, hs), rotated already for RoPE models; k_cache: (B, T_cap, H, N, hs);
    v_cache: (B, T_cap, H, dv) (strided views, innermost dim contiguous).  Returns
    (B, Tq, H*dv): rows ``pos:`` of ``diff_attention`` over the same ``pos + Tq``
    positions, with nothing saved for a backward.  Cache rows past ``pos + Tq`` may hold
    anything.  Raises for a shape without a kernel plan (``extend_supported``): there is
    no fallback here."""
    lib = _lib.load()
    _require_gpu(q, k_cache, v_cache, coef)
    if q.dim() != 5:
        raise RuntimeError("q must be (B, Tq, H, N, hs)")
    B, Tq, H, N, hs = q.shape
    T_cap = _cache_shapes(q, k_cache, v_cache)
    _cache_dtype(q, k_cache, v_cache)
    _coef_shape(coef, H, N)
    pos = int(pos)
    if pos < 0 or pos + Tq > T_cap:
        raise RuntimeError(f"extend rows {pos}..{pos + Tq - 1} outside the cache's {T_cap} rows")
    return _extend(lib, q, k_cache, v_cache, coef, T_cap, pos=pos)


# ------------------------------------------------------------------ ragged ---
def diff_attention_decode_ragged(q: Tensor, k_cache: Tensor, v_cache: Tensor, coef: Tensor, lengths: Tensor,
                                 max_length: Optional[int] = None) -> Tensor:
    """``diff_attention_decode`` for a batch whose sequences sit at different lengths:
    o[b] = sum_i coef[h,i] softmax(q_i[b] K_i[b, :len_b]^T / sqrt(hs)) V[b, :len_b], len_b = lengths[b].

    q, k_cache, v_cache, coef as for ``diff_attention_decode``; ``lengths``: device int32
    (B,), read by the kernels (no host sync).  ``max_length``: a host upper bound of every
    length, which sizes the grid; default T_cap.  The kernels clamp each length to
    [0, max_length]; a sequence of length 0 gets zeros; cache rows past a sequence's
    length may hold anything.  With all lengths equal to L the result is bitwise that of
    ``diff_attention_decode(..., L)``, whatever ``max_length``.  Returns (B, H*dv)."""
    lib = _lib.load()
    _require_gpu(q, k_cache, v_cache, coef)
    B, H, N, hs = q.shape
    T_cap = _cache_shapes(q, k_cache, v_cache)
    max_length = _decode_bound(max_length, T_cap)
    _cache_dtype(q, k_cache, v_cache)
    _batch_int32(lengths, B, q, "lengths")
    return _decode(lib, q, k_cache, v_cache, coef, max_length, T_cap, lengths=lengths)


def diff_attention_extend_ragged(q: Tensor, k_cache: Tensor, v_cache: Tensor, coef: Tensor, pos: Tensor,
                                 counts: Optional[Tensor] = None, *, _rows: bool = False) -> Tensor:
    """``diff_attention_extend`` for a batch whose sequences sit at different positions:
    sequence b appends ``counts[b]`` real rows at absolute position ``pos[b]``; row r <
    counts[b] is ``diff_attention_extend``'s row at pos = pos[b], rows r >= counts[b] are
    zeros (padding; those q rows are never read).

    q: (B, Tq, H, N, hs) padded; caches as for ``diff_attention_extend``, with rows
    0 .. pos[b]+counts[b]-1 of sequence b valid and everything above arbitrary.  ``pos``,
    ``counts``: device int32 (B,), read by the kernel (no host sync); ``counts=None``:
    Tq for every sequence.  The kernel clamps pos[b] to [0, T_cap - Tq] and counts[b] to
    [0, Tq].  With all pos equal and ``counts=None`` the result is bitwise that of
    ``diff_attention_extend``.  Returns (B, Tq, H*dv).  No fallback: raises for a shape
    without a kernel plan (``extend_supported``)."""
    lib = _lib.load()
    _require_gpu(q, k_cache, v_cache, coef)
    if q.dim() != 5:
        raise RuntimeError("q must be (B, Tq, H, N, hs)")
    B, Tq, H, N, hs = q.shape
    T_cap = _cache_shapes(q, k_cache, v_cache)
    _cache_dtype(q, k_cache, v_cache)
    _step_operands(q, coef, pos, counts, T_cap, "cache")
    return _extend(lib, q, k_cache, v_cache, coef, T_cap, pos_dev=pos, counts=counts, rows=_rows)


# ------------------------------------------------------------------- paged ---
PAGE_SIZES = (32, 64, 128, 256)


def _table_pages(block_table: Tensor, B: int, q: Tensor) -> int:
    """Checks of a step's block table; returns max_pages."""
    if (not isinstance(block_table, Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2
            or block_table.shape[0] != B or block_table.shape[1] < 1 or block_table.device != q.device):
        raise RuntimeError(f"block_table must be a device int32 tensor of shape ({B}, max_pages) on {q.device}")
    if not block_table.is_contiguous():
        raise RuntimeError("block_table must be contiguous")
    return block_table.shape[1]


def _page_tuple(q: Tensor, k_pool: Tensor, v_pool: Tensor, scale_pool: Optional[Tensor], block_table: Tensor):
    """Checks of the pool views (``scale_pool`` given: the fp8 ones, ``_fp8_views``) against q
    (B, [Tq,] H, N, hs) and of the block table, shared by every paged op.  Returns ``_decode`` /
    ``_extend``'s ``page`` = (block_table, P, max_pages, n_pages), T_cap and dv."""
    B, (H, N, hs) = q.shape[0], tuple(q.shape[-3:])
    if scale_pool is not None:
        n_pages, P, Hp, Np, hsp, dv = _fp8_views(k_pool, v_pool, scale_pool)
        if (Hp, Np, hsp) != (H, N, hs) or k_pool.device != q.device:
            raise RuntimeError("the pool views do not match q")
    else:
        if k_pool.dim() != 5 or v_pool.dim() != 4:
            raise RuntimeError("k_pool must be (n_pages, P, H, N, hs) and v_pool (n_pages, P, H, dv)")
        n_pages, P, dv = k_pool.shape[0], k_pool.shape[1], v_pool.shape[-1]
        if P not in PAGE_SIZES:
            raise RuntimeError(f"page size {P} is not one of {PAGE_SIZES}")
        if n_pages < 1:
            raise RuntimeError("the pool holds no page")
        if tuple(k_pool.shape) != (n_pages, P, H, N, hs) or tuple(v_pool.shape) != (n_pages, P, H, dv):
            raise RuntimeError("k_pool/v_pool shapes do not match q")
        if q.dtype != k_pool.dtype or q.dtype != v_pool.dtype:
            raise RuntimeError("q, k_pool and v_pool must share a dtype")
    max_pages = _table_pages(block_table, B, q)
    return (block_table, P, max_pages, n_pages), max_pages * P, dv


def _decode_paged(lib, q: Tensor, k_pool: Tensor, v_pool: Tensor, scale_pool: Optional[Tensor], coef: Tensor,
                  block_table: Tensor, lengths: Tensor, max_length: Optional[int], plan=None) -> Tensor:
    """The body of the four paged decode ops (``scale_pool``: the fp8 ones; ``plan``: the shared-prefix
    ones, checked by their caller), after their own library and device checks."""
    B, H = q.shape[:2]
    page, T_cap, dv = _page_tuple(q, k_pool, v_pool, scale_pool, block_table)
    max_length = _decode_bound(max_length, T_cap)
    _batch_int32(lengths, B, q, "lengths")
    if plan is not None and B == 0:
        return q.new_empty(0, H * dv)            # an empty batch (its tensors have no address to pass)
    return _decode(lib, q, k_pool, v_pool, coef, max_length, T_cap, lengths=lengths, page=page,
                   scale_pool=scale_pool, plan=plan)


def _extend_paged(lib, q: Tensor, k_pool: Tensor, v_pool: Tensor, scale_pool: Optional[Tensor], coef: Tensor,
                  block_table: Tensor, pos: Tensor, counts: Optional[Tensor], rows: bool) -> Tensor:
    """The body of the paged extend ops and, with ``rows``, of the paged multi-row decode ops
    (``scale_pool``: the fp8 ones), after their own library and device checks."""
    if q.dim() != 5:
        raise RuntimeError("q must be (B, Tq, H, N, hs)")
    page, T_cap, _ = _page_tuple(q, k_pool, v_pool, scale_pool, block_table)
    _step_operands(q, coef, pos, counts, T_cap, "table")
    return _extend(lib, q, k_pool, v_pool, coef, T_cap, pos_dev=pos, counts=counts, page=page,
                   scale_pool=scale_pool, rows=rows)


def diff_attention_decode_paged(q: Tensor, k_pool: Tensor, v_pool: Tensor, coef: Tensor, block_table: Tensor,
                                lengths: Tensor, max_length: Optional[int] = None) -> Tensor:
    """``diff_attention_decode_ragged`` over a paged cache: key row j of sequence b is
    row ``j % P`` of pool page ``block_table[b, j // P]``.

    q: (B, H, N, hs); k_pool: (n_pages, P, H, N, hs); v_pool: (n_pages, P, H, dv) (strided
    views of one packed pool, innermost dim contiguous), P in 32, 64, 128, 256;
    ``block_table``: contiguous device int32 (B, max_pages); ``lengths``: device int32 (B,).
    The logical capacity is T_cap = max_pages * P, and ``max_length`` (default T_cap) the
    host upper bound of every length.  Only table entries below ceil(lengths[b] / P) are
    read (the rest may hold anything, e.g. -1) and every id read is clamped into the pool;
    rows past a length and pages nobody names may hold NaN.  Cut a contiguous cache
    (B, T_cap, ...) into pages placed anywhere in the pool: the result is bitwise that of
    ``diff_attention_decode_ragged`` on the contiguous cache.  Returns (B, H*dv)."""
    lib = _lib.load()
    _require_gpu(q, k_pool, v_pool, coef)
    B, H, N, hs = q.shape
    return _decode_paged(lib, q, k_pool, v_pool, None, coef, block_table, lengths, max_length)


def diff_attention_extend_paged(q: Tensor, k_pool: Tensor, v_pool: Tensor, coef: Tensor, block_table: Tensor,
                                pos: Tensor, counts: Optional[Tensor] = None, *, _rows: bool = False) -> Tensor:
    """``diff_attention_extend_ragged`` over a paged cache (pool views and ``block_table``
    as for ``diff_attention_decode_paged``): sequence b appends ``counts[b]`` real rows at
    ``pos[b]``, its cache rows 0 .. pos[b]+counts[b]-1 reached through its table row
    (entries below ceil((pos[b] + counts[b]) / P) are read).  q: (B, Tq, H, N, hs) padded;
    rows r >= counts[b] come back as zeros.  The kernel clamps pos[b] to
    [0, max_pages * P - Tq].  Bitwise equal to ``diff_attention_extend_ragged`` on the
    gathered contiguous cache.  Returns (B, Tq, H*dv).  No fallback: raises for a shape
    without a kernel plan (``extend_supported``)."""
    lib = _lib.load()
    _require_gpu(q, k_pool, v_pool, coef)
    return _extend_paged(lib, q, k_pool, v_pool, None, coef, block_table, pos, counts, _rows)


# --------------------------------------------------------------- fp8 pages ---
# The paged cache with one byte per element (include/diffattn.h "FP8 paged KV cache"):
# OCP e4m3fn bytes in today's row layout [K (H, N, hs) | V (H, dv)] and one fp32 scale per
# (row, head, K_i | V) in scale_pool (n_pages, P, H, N + 1), index N holding V's scale.
FP8_MAX = 448.0


def fp8_cache_supported() -> bool:
    """Whether the loaded library has the fp8-cache entry points (an older build of the
    same ABI may not)."""
    return _lib.fp8_symbols(_lib.load())


def kv_quant_reference(x: Tensor) -> Tuple[Tensor, Tensor]:
    """The cache's quantiser in plain torch (any device), over the last dimension of ``x``:
    amax = max|x| in fp32 of the values as stored, scale = amax / 448, byte =
    e4m3fn_rne(clamp(x / scale, -448, 448)); a zero vector gives scale 0 and bytes 0.  The
    clamp precedes the conversion (torch's own conversion turns 500.0 into NaN).
    Returns (uint8 bytes shaped like ``x``, fp32 scales shaped like ``x[..., 0]``)."""
    xf = x.detach().to(torch.float32)
    amax = xf.abs().amax(dim=-1)
    scale = amax / FP8_MAX
    safe = torch.where(amax > 0, scale, torch.ones_like(scale))
    y = (xf / safe[..., None]).clamp_(-FP8_MAX, FP8_MAX)
    y = torch.where(amax[..., None] > 0, y, torch.zeros_like(y))
    return y.to(torch.float8_e4m3fn).view(torch.uint8), scale


def kv_dequant_reference(k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor, table_row, length: int):
    """Rows 0 .. length-1 of one sequence, gathered through its block-table row and
    dequantised (x^ = float(byte) * scale) in plain torch on the pools' device.
    k_pool_u8 (n_pages, P, H, N, hs), v_pool_u8 (n_pages, P, H, dv), scale_pool (n_pages, P,
    H, N + 1); ``table_row``: the sequence's page ids (a tensor or a list; entries past
    ceil(length / P) are not looked at).  Returns fp32 (k (length, H, N, hs), v (length, H, dv))."""
    P = k_pool_u8.shape[1]
    n = -(-int(length) // P)
    pages = torch.as_tensor(table_row)[:n].to(device=k_pool_u8.device, dtype=torch.long)
    k = k_pool_u8.index_select(0, pages).flatten(0, 1)[:length].contiguous().view(torch.float8_e4m3fn).float()
    v = v_pool_u8.index_select(0, pages).flatten(0, 1)[:length].contiguous().view(torch.float8_e4m3fn).float()
    s = scale_pool.index_select(0, pages).flatten(0, 1)[:length].float()
    N = k.shape[2]
    return k * s[..., :N, None], v * s[..., N, None]


def _fp8_views(k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor):
    """Checks of the three fp8 pool views; returns (n_pages, P, H, N, hs, dv)."""
    if k_pool_u8.dim() != 5 or v_pool_u8.dim() != 4 or scale_pool.dim() != 4:
        raise RuntimeError("k_pool_u8 must be (n_pages, P, H, N, hs), v_pool_u8 (n_pages, P, H, dv) and "
                           "scale_pool (n_pages, P, H, N + 1)")
    n_pages, P, H, N, hs = k_pool_u8.shape
    dv = v_pool_u8.shape[-1]
    if k_pool_u8.dtype != torch.uint8 or v_pool_u8.dtype != torch.uint8 or scale_pool.dtype != torch.float32:
        raise RuntimeError("the fp8 pools are uint8 views and the scale pool is fp32")
    if P not in PAGE_SIZES:
        raise RuntimeError(f"page size {P} is not one of {PAGE_SIZES}")
    if n_pages < 1:
        raise RuntimeError("the pool holds no page")
    if tuple(v_pool_u8.shape) != (n_pages, P, H, dv) or tuple(scale_pool.shape) != (n_pages, P, H, N + 1):
        raise RuntimeError("v_pool_u8 / scale_pool shapes do not match k_pool_u8")
    if scale_pool.stride()[1:] != (H * (N + 1), N + 1, 1):
        raise RuntimeError("the scales of a page must be contiguous")
    if k_pool_u8.device != v_pool_u8.device or k_pool_u8.device != scale_pool.device:
        raise RuntimeError("the pools must share a device")
    return n_pages, P, H, N, hs, dv


def diff_attention_decode_paged_fp8(q: Tensor, k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor,
                                    coef: Tensor, block_table: Tensor, lengths: Tensor,
                                    max_length: Optional[int] = None) -> Tensor:
    """``diff_attention_decode_paged`` over an fp8 page pool: the kernel reads e4m3fn bytes
    and their scales and never materialises the dequantised rows; every sum is fp32.

    q: (B, H, N, hs) bf16 / f16 / f32 (the dtype of the result); k_pool_u8 (n_pages, P, H, N,
    hs) and v_pool_u8 (n_pages, P, H, dv): uint8 views of one packed byte pool; scale_pool
    (n_pages, P, H, N + 1) fp32, contiguous inside a page.  ``block_table``, ``lengths``,
    ``max_length``, clamps, zeros for an empty sequence: as ``diff_attention_decode_paged``;
    rows past a length and pages nobody names may hold any bytes and any scales, NaN and
    Inf included.  Returns (B, H*dv).  No fallback: raises if the library lacks the entry
    point (``fp8_cache_supported``)."""
    lib = _lib.load()
    if not _lib.fp8_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no fp8-cache entry points (fp8_cache_supported)")
    _require_gpu(q, k_pool_u8, v_pool_u8, scale_pool, coef)
    B, H, N, hs = q.shape
    return _decode_paged(lib, q, k_pool_u8, v_pool_u8, scale_pool, coef, block_table, lengths, max_length)


def extend_fp8_supported(dtype: torch.dtype, hs: int, N: int, dv: int) -> bool:
    """Whether ``diff_attention_extend_paged_fp8`` has a kernel plan for this shape
    (dta_extend_fp8_supported): what both ``extend_supported`` and ``kv_quant_rows`` take, hs % 16
    == 0 in 16..128, dv % 32 == 0 up to 256, N <= 4.  False on a library without the entry points."""
    lib = _lib.load()
    return _lib.fp8_extend_symbols(lib) and bool(lib.dta_extend_fp8_supported(_lib.dtype_code(dtype), hs, N, dv))


def diff_attention_extend_paged_fp8(q: Tensor, k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor,
                                    coef: Tensor, block_table: Tensor, pos: Tensor,
                                    counts: Optional[Tensor] = None, *, _rows: bool = False) -> Tensor:
    """``diff_attention_extend_paged`` over an fp8 page pool, one launch: sequence b appends
    ``counts[b]`` real rows at ``pos[b]`` against its dequantised cache rows 0 ..
    pos[b]+counts[b]-1 (the new rows' own bytes and scales already written, ``kv_quant_rows``).
    The kernel converts the bytes while it stages a key tile: q_i times the exact byte values
    on the MFMA, the fp32 scores times the key's K_i scale, V staged as byte * scale rounded
    once to q's dtype (exact in fp32).

    q: (B, Tq, H, N, hs) bf16 / f16 / f32 padded (the dtype of the result); pools, scales and
    ``block_table`` as for ``diff_attention_decode_paged_fp8``; ``pos``, ``counts``, the clamps
    and the zero rows r >= counts[b] as for ``diff_attention_extend_paged``.  Rows past
    pos[b]+counts[b] and pages nobody names may hold any bytes and any scales, NaN and Inf
    included.  Returns (B, Tq, H*dv).  No fallback: raises for a shape without a kernel plan
    or a library without the entry point (``extend_fp8_supported``)."""
    lib = _lib.load()
    if not _rows and not _lib.fp8_extend_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no fp8 extend entry points (extend_fp8_supported)")
    _require_gpu(q, k_pool_u8, v_pool_u8, scale_pool, coef)
    return _extend_paged(lib, q, k_pool_u8, v_pool_u8, scale_pool, coef, block_table, pos, counts, _rows)


# ------------------------------------------------- short multi-row steps ---
# The same step as the ragged extend ops (arguments, checks, clamps, zero padding rows) on the
# split-key decode plan: one split launch and one combine launch for 1 .. 8 rows per sequence,
# every cached row loaded once.  Each real row is bitwise the matching one-row decode op at
# lengths = pos + r + 1.
DECODE_ROWS_MAX = 8


def decode_rows_supported(dtype: torch.dtype, hs: int, N: int, dv: int, Tq: int, fp8: bool = False) -> bool:
    """Whether ``diff_attention_decode_rows`` (``fp8``: ``..._paged_fp8``) has a kernel plan
    (dta_decode_rows_supported): the split-key shapes -- (hs, dv) in (32, 64), (64, 128), (128, 256)
    with N <= 4, or N = 1 with dv = hs in 64, 128 -- at 1 <= Tq <= 8.  False on a library
    without the entry points."""
    lib = _lib.load()
    return _lib.rows_symbols(lib) and bool(
        lib.dta_decode_rows_supported(_lib.dtype_code(dtype), hs, N, dv, Tq, int(bool(fp8))))


def diff_attention_decode_rows(q: Tensor, k_cache: Tensor, v_cache: Tensor, coef: Tensor, pos: Tensor,
                               counts: Optional[Tensor] = None) -> Tensor:
    """``diff_attention_extend_ragged``'s step -- q (B, Tq, H, N, hs) padded, ``pos`` / ``counts``
    device int32 (B,), zeros for rows r >= counts[b] -- for 1 <= Tq <= 8 on the split-key decode
    plan.  Row r < counts[b] of sequence b is bitwise ``diff_attention_decode_ragged`` at
    lengths[b] = pos[b] + r + 1.  Cache rows >= pos[b] + counts[b] are never loaded.  Returns
    (B, Tq, H*dv).  No fallback: raises without a plan (``decode_rows_supported``)."""
    return diff_attention_extend_ragged(q, k_cache, v_cache, coef, pos, counts, _rows=True)


def diff_attention_decode_rows_paged(q: Tensor, k_pool: Tensor, v_pool: Tensor, coef: Tensor, block_table: Tensor,
                                     pos: Tensor, counts: Optional[Tensor] = None) -> Tensor:
    """``diff_attention_decode_rows`` over a paged cache (arguments of
    ``diff_attention_extend_paged``); row r is bitwise ``diff_attention_decode_paged`` at
    lengths[b] = pos[b] + r + 1.  Table entries >= ceil((pos[b] + counts[b]) / P) are not read."""
    return diff_attention_extend_paged(q, k_pool, v_pool, coef, block_table, pos, counts, _rows=True)


def diff_attention_decode_rows_paged_fp8(q: Tensor, k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor,
                                         coef: Tensor, block_table: Tensor, pos: Tensor,
                                         counts: Optional[Tensor] = None) -> Tensor:
    """``diff_attention_decode_rows_paged`` over an fp8 page pool (arguments of
    ``diff_attention_extend_paged_fp8``); row r is bitwise ``diff_attention_decode_paged_fp8`` at
    lengths[b] = pos[b] + r + 1.  Scales of rows >= pos[b] + counts[b] are not read."""
    return diff_attention_extend_paged_fp8(q, k_pool_u8, v_pool_u8, scale_pool, coef, block_table, pos, counts,
                                           _rows=True)


def kv_quant_rows(k_new: Tensor, v_new: Tensor, k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor,
                  slots: Tensor) -> None:
    """Quantise the new rows of a step into an fp8 page pool (``kv_quant_reference``'s
    arithmetic, one launch): k_new (B, Tn, H, N, hs) and v_new (B, Tn, H, dv) are strided
    views in the activation dtype (K may be the RoPE temporary, V a slice of the packed
    projection); row (b, t) goes to row ``slots[b * Tn + t] % P`` of page ``slots[..] // P``.
    The pool views hold the pool's pages and, last, the spare page the padding rows of a
    step point into; ``slots``: contiguous device int32 (B * Tn,), clamped into the views by
    the kernel.  Writes the bytes and the N + 1 scales of the named rows, nothing else.
    hs and dv must be multiples of 16 (``RuntimeError`` otherwise: there is no fallback)."""
    lib = _lib.load()
    if not _lib.fp8_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no fp8-cache entry points (fp8_cache_supported)")
    _require_gpu(k_new, v_new, k_pool_u8, v_pool_u8, scale_pool, slots)
    if k_new.dim() != 5 or v_new.dim() != 4:
        raise RuntimeError("k_new must be (B, Tn, H, N, hs) and v_new (B, Tn, H, dv)")
    B, Tn, H, N, hs = k_new.shape
    n_all, P, Hp, Np, hsp, dv = _fp8_views(k_pool_u8, v_pool_u8, scale_pool)
    if (Hp, Np, hsp) != (H, N, hs) or tuple(v_new.shape) != (B, Tn, H, dv) or k_new.dtype != v_new.dtype:
        raise RuntimeError("k_new / v_new do not match each other or the pool views")
    if n_all < 2:
        raise RuntimeError("the pool views must hold at least one page and the spare page")
    if (slots.dtype != torch.int32 or tuple(slots.shape) != (B * Tn,) or not slots.is_contiguous()
            or slots.device != k_new.device or k_pool_u8.device != k_new.device):
        raise RuntimeError(f"slots must be a contiguous device int32 tensor of shape ({B * Tn},) on {k_new.device}")
    if B * Tn == 0:
        return                                  # no rows to write (an empty ``slots`` has no address to pass)
    a = _lib.KvQuantRowsArgs(_lib.dtype_code(k_new.dtype), B, Tn, H, N, hs, dv, P, n_all - 1,
                             _lib.tensor5(k_new), _lib.tensor5(v_new), _lib.tensor5(k_pool_u8),
                             _lib.tensor5(v_pool_u8), scale_pool.data_ptr(), scale_pool.stride(0), slots.data_ptr())
    _lib.check(lib.dta_kv_quant_rows(a, _lib.stream_handle(k_new.device)))


# ------------------------------------------------- fused step row write ---
def kv_step_supported() -> bool:
    """Whether the loaded library has ``dta_kv_step_rows`` (an older build of the same ABI may not)."""
    return _lib.step_symbols(_lib.load())


def kv_step_rows(q: Tensor, k_new: Tensor, v_new: Tensor, pos: Tensor, counts: Tensor, t_cap: int,
                 freqs: Optional[Tensor], dest=None, block_table: Optional[Tensor] = None,
                 page_size: Optional[int] = None, n_pages: Optional[int] = None):
    """The RoPE and the cache scatter of a step's rows at per-sequence positions, in one launch
    (``dta_kv_step_rows``).  q, k_new (B, Tn, H, N, hs) and v_new (B, Tn, H, dv) are the strided
    views of the packed projection (``split_packed``); row r of sequence b sits at
    ``at = pos[b] + r`` and is real if ``r < counts[b] and at < t_cap`` (pos, counts: device int32
    (B,)).  ``freqs``: the whole RoPE table fp32 (t_cap, hs/2, 2), or None.

    With a table every row of q, padding rows included, is rotated to row ``min(at, t_cap - 1)``
    into a new tensor, and K_i of a real row to row ``at``, bitwise ``rope_rows``.  K_i and V of a
    real row are stored to the row's place; a padding row stores no K and no V anywhere:

    * ``dest=(k_rows, v_rows)`` (B, t_cap, H, N, hs) / (B, t_cap, H, dv): row ``at`` of sequence b;
    * ``dest=(k_pool, v_pool)`` (n_pages, P, ...) with ``block_table`` (B, max_pages): row
      ``at % P`` of page ``block_table[b, at // P]`` (the id is clamped into the views);
    * ``dest=None`` with ``block_table``, ``page_size`` and ``n_pages`` (an fp8 pool): no pool is
      written; the rotated K_i goes to a (B, Tn, H, N, hs) temporary and ``slots`` int32 (B * Tn,)
      gets ``page * P + at % P`` (a padding row: ``n_pages * P + at % P``, in the spare page) --
      what ``kv_quant_rows`` takes next.

    Returns ``(q_rot, k_out, slots)``: q_rot None without a table (keep ``q``); k_out None unless
    ``dest`` is None and there is a table (without one ``k_new`` is what to quantise); slots None
    unless ``dest`` is None.  hs and dv multiples of 8 up to 128 / 256, N <= 8 (``RuntimeError``
    otherwise: there is no fallback)."""
    lib = _lib.load()
    if not _lib.step_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no dta_kv_step_rows (kv_step_supported)")
    _require_gpu(q, k_new, v_new, pos, counts)
    if q.dim() != 5 or k_new.dim() != 5 or v_new.dim() != 4:
        raise RuntimeError("q and k_new must be (B, Tn, H, N, hs) and v_new (B, Tn, H, dv)")
    B, Tn, H, N, hs = k_new.shape
    dv = v_new.shape[-1]
    if tuple(q.shape) != (B, Tn, H, N, hs) or tuple(v_new.shape) != (B, Tn, H, dv):
        raise RuntimeError("q, k_new and v_new do not match each other")
    if not (q.dtype == k_new.dtype == v_new.dtype):
        raise RuntimeError("q, k_new and v_new must share a dtype")
    t_cap = int(t_cap)
    if t_cap < 1:
        raise RuntimeError(f"t_cap {t_cap} < 1")
    _batch_int32(pos, B, k_new, "pos")
    _batch_int32(counts, B, k_new, "counts")
    dev = k_new.device
    if freqs is not None:
        _require_gpu(freqs)
        if (freqs.dtype != torch.float32 or tuple(freqs.shape) != (t_cap, hs // 2, 2) or not freqs.is_contiguous()
                or freqs.device != dev):
            raise RuntimeError(f"freqs must be the whole contiguous fp32 table ({t_cap}, {hs // 2}, 2) on {dev}")
    kind, P, max_pages, pages = _lib.KV_STEP_CONTIGUOUS, 0, 0, 0
    if block_table is not None:
        max_pages = _table_pages(block_table, B, k_new)
    if dest is None:
        kind = _lib.KV_STEP_SLOTS
        if block_table is None or page_size not in PAGE_SIZES or n_pages is None or int(n_pages) < 1:
            raise RuntimeError(f"dest=None needs block_table, a page_size of {PAGE_SIZES} and n_pages >= 1")
        P, pages = int(page_size), int(n_pages)
        k_dst = v_dst = None
    else:
        k_dst, v_dst = dest
        _require_gpu(k_dst, v_dst)
        if k_dst.dim() != 5 or v_dst.dim() != 4 or k_dst.dtype != k_new.dtype or v_dst.dtype != k_new.dtype \
                or k_dst.device != dev or v_dst.device != dev:
            raise RuntimeError("dest must be (k, v) views of 5 and 4 dimensions in the rows' dtype, on their device")
        if block_table is None:
            if tuple(k_dst.shape) != (B, t_cap, H, N, hs) or tuple(v_dst.shape) != (B, t_cap, H, dv):
                raise RuntimeError("the cache views must be (B, t_cap, H, N, hs) and (B, t_cap, H, dv)")
        else:
            kind = _lib.KV_STEP_PAGED
            pages, P = k_dst.shape[0], k_dst.shape[1]
            if P not in PAGE_SIZES or pages < 1:
                raise RuntimeError(f"page size {P} is not one of {PAGE_SIZES}, or the pool holds no page")
            if tuple(k_dst.shape) != (pages, P, H, N, hs) or tuple(v_dst.shape) != (pages, P, H, dv):
                raise RuntimeError("the pool views must be (n_pages, P, H, N, hs) and (n_pages, P, H, dv)")
    if kind != _lib.KV_STEP_CONTIGUOUS and max_pages * P < t_cap:
        raise RuntimeError(f"a table of {max_pages} pages of {P} rows does not reach t_cap {t_cap}")
    q_rot = k_out = slots = None
    if freqs is not None:
        q_rot = torch.empty(B, Tn, H, N, hs, device=dev, dtype=q.dtype)
    if kind == _lib.KV_STEP_SLOTS:
        slots = torch.empty(B * Tn, device=dev, dtype=torch.int32)
        if freqs is not None:
            k_out = torch.empty(B, Tn, H, N, hs, device=dev, dtype=q.dtype)
        k_dst = k_out
    if B * Tn == 0:
        return q_rot, k_out, slots
    none = _lib.DtaTensor()
    view = lambda t: none if t is None else _lib.tensor5(t)          # noqa: E731
    a = _lib.KvStepRowsArgs(_lib.dtype_code(q.dtype), B, Tn, H, N, hs, dv, t_cap, kind, P, max_pages, pages,
                            _lib.tensor5(q), _lib.tensor5(k_new), _lib.tensor5(v_new), view(q_rot), view(k_dst),
                            view(v_dst), _lib.ptr(freqs), pos.data_ptr(), counts.data_ptr(), _lib.ptr(block_table),
                            _lib.ptr(slots))
    _lib.check(lib.dta_kv_step_rows(a, _lib.stream_handle(dev)))
    return q_rot, k_out, slots


# ------------------------------------------------------------------ sampling ---
# One token per logits row: temperature, top-k, top-p and a counter-based uniform (Philox4x32-10 of
# (seed, stream, offset)), so a row's token depends on the row, its parameters and that triple only --
# not on the batch it is sampled in.  The definition is include/diffattn.h's ("Sampling");
# ``sample_rows`` is the HIP kernel, ``sample_rows_reference`` the same definition in torch.
SAMPLE_MAX_V = 1 << 20
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def sample_supported() -> bool:
    """Whether the loaded library has ``dta_sample_rows`` (an older build of the same ABI may not)."""
    return _lib.sample_symbols(_lib.load())


def _mulhilo32(a: int, b: Tensor) -> Tuple[Tensor, Tensor]:
    """(high, low) 32-bit halves of a * b for a 32-bit constant and an int64 tensor of 32-bit values,
    through 16-bit halves of b so that nothing passes 2^63."""
    p0, p1 = a * (b & 0xFFFF), a * (b >> 16)
    low = p0 + ((p1 & 0xFFFF) << 16)
    return (p1 >> 16) + (low >> 32), low & _M32


def philox4x32_10(counter: Tensor, key: Tensor) -> Tensor:
    """Philox4x32-10 in integer tensor ops: counter (..., 4) and key (..., 2), int64 tensors holding
    32-bit words; returns the four output words (..., 4)."""
    c0, c1, c2, c3 = (counter[..., i] & _M32 for i in range(4))
    k0, k1 = key[..., 0] & _M32, key[..., 1] & _M32
    for _ in range(10):
        h0, l0 = _mulhilo32(_PHILOX_M0, c0)
        h1, l1 = _mulhilo32(_PHILOX_M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return torch.stack((c0, c1, c2, c3), dim=-1)


def sample_uniform(seed: int, stream: Tensor, offset: Tensor) -> Tensor:
    """The sampler's uniform, fp64 in [0, 1): ``(out[0] >> 8) * 2^-24`` of Philox4x32-10 with key
    (seed lo, seed hi) and counter (offset lo, offset hi, stream lo, stream hi); stream and offset are
    int64 tensors of one shape (read as unsigned 64-bit)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    halves = lambda t: (t & _M32, (t >> 32) & _M32)                    # noqa: E731
    counter = torch.stack(halves(offset) + halves(stream), dim=-1)
    key = torch.tensor([seed & _M32, seed >> 32], dtype=torch.int64, device=stream.device).expand(*stream.shape, 2)
    return (philox4x32_10(counter, key)[..., 0] >> 8).double() * 2.0 ** -24


def _sample_rows_2d(logits: Tensor) -> Tensor:
    if not isinstance(logits, Tensor) or logits.dim() < 1 or logits.shape[-1] < 1:
        raise RuntimeError("logits must be (..., V) with V >= 1")
    if logits.dtype not in _lib._DTYPES:
        raise RuntimeError(f"logits must be bf16, fp16 or fp32, got {logits.dtype}")
    if logits.shape[-1] > SAMPLE_MAX_V:
        raise RuntimeError(f"V {logits.shape[-1]} is above {SAMPLE_MAX_V}")
    x = logits if logits.dim() == 2 else logits.reshape(-1, logits.shape[-1])
    return x if x.stride(1) == 1 or x.shape[1] == 1 else x.contiguous()


def _sample_param(v, R: int, dtype, device, name: str):
    """A sampling parameter as (scalar, per-row tensor or None)."""
    if isinstance(v, Tensor):
        if v.numel() != R or v.device != device:
            raise RuntimeError(f"{name} must be a scalar or a tensor of {R} entries on {device}")
        return None, v.reshape(R).to(dtype).contiguous()
    v = float(v) if dtype.is_floating_point else int(v)
    if v != v:
        raise RuntimeError(f"{name} is NaN")
    return v, None


def _sample_counter(v, R: int, device, name: str) -> Optional[Tensor]:
    if v is None:
        return None
    if not isinstance(v, Tensor):
        return torch.full((R,), int(v), dtype=torch.int64, device=device)
    if v.numel() != R or v.device != device or v.dtype != torch.int64:
        raise RuntimeError(f"{name} must be an int64 tensor of {R} entries on {device}")
    return v.reshape(R).contiguous()


def sample_rows_reference(logits: Tensor, temperature=1.0, top_k=0, top_p=1.0, seed: int = 0, stream=None,
                          offset=None, return_logprobs: bool = False, kept_only: bool = False):
    """``sample_rows`` in torch, on the logits' device: the same definition with fp64 weights and
    sums (so a token may differ from the kernel's where ``u * Z`` falls within rounding of a CDF
    step).  The tests' oracle, and what ``sample_rows`` runs on CPU tensors and on a library without
    ``dta_sample_rows``.  ``kept_only``: return instead the bool mask, shaped like ``logits``, of what
    top-k and top-p keep (all False for a greedy or a degenerate row)."""
    x2 = _sample_rows_2d(logits)
    R, V = x2.shape
    dev = x2.device
    as_rows = lambda s, t, dt: t.to(dt) if t is not None else torch.full((R,), s, dtype=dt, device=dev)   # noqa: E731
    T = as_rows(*_sample_param(temperature, R, torch.float32, dev, "temperature"), torch.float32).double()
    k = as_rows(*_sample_param(top_k, R, torch.int32, dev, "top_k"), torch.int64)
    p = as_rows(*_sample_param(top_p, R, torch.float32, dev, "top_p"), torch.float32).double()
    strm = _sample_counter(stream, R, dev, "stream")
    strm = torch.arange(R, dtype=torch.int64, device=dev) if strm is None else strm
    off = _sample_counter(offset, R, dev, "offset")
    off = torch.zeros(R, dtype=torch.int64, device=dev) if off is None else off
    x = x2.float().double()
    ninf = float("-inf")
    bad = torch.isnan(x).any(1) | (x == float("inf")).any(1) | (x == ninf).all(1)
    x = torch.where(bad[:, None], torch.zeros_like(x), x)              # any finite row: the result is overwritten
    cols = torch.arange(V, device=dev)
    m = x.max(dim=1, keepdim=True).values
    amax = torch.where(x == m, cols, V).min(dim=1).values
    greedy = torch.isnan(T) | (T <= 0)
    T = torch.where(greedy, torch.ones_like(T), T)
    z = (x - m) / T[:, None]
    w = torch.exp(z)
    # top-k: the k-th largest value and everything that ties with it
    xs, order = torch.sort(x, dim=1, descending=True, stable=True)
    k_on = (k > 0) & (k < V)
    kth = xs.gather(1, (torch.where(k_on, k, V) - 1)[:, None])
    kept = x >= kth
    # top-p among those: G_i = the kept weight strictly above x_i, taken at the head of its tie class
    ws = torch.where(kept, w, torch.zeros_like(w)).gather(1, order)
    above = ws.cumsum(1) - ws
    head = torch.ones_like(xs, dtype=torch.bool)
    head[:, 1:] = xs[:, 1:] != xs[:, :-1]
    G = torch.where(head, above, torch.zeros_like(above)).cummax(dim=1).values
    Zk = ws.sum(1, keepdim=True)
    p_on = (p > 0) & (p < 1)
    in_p = torch.zeros_like(kept).scatter(1, order, G < p[:, None] * Zk)
    kept = kept & (in_p | ~p_on[:, None])
    if kept_only:
        return (kept & ~greedy[:, None] & ~bad[:, None]).reshape(logits.shape)
    wk = torch.where(kept, w, torch.zeros_like(w))
    Z = wk.sum(1)
    C = wk.cumsum(1)
    u = sample_uniform(seed, strm, off)
    hit = kept & (C > (u * Z)[:, None])
    tok = torch.where(hit, cols, V).min(dim=1).values
    last = torch.where(kept, cols, -1).max(dim=1).values
    tok = torch.where(tok == V, last, tok)
    lp = z.gather(1, tok[:, None])[:, 0] - torch.log(Z)
    lp_greedy = -torch.log(w.sum(1))
    tok = torch.where(greedy, amax, tok)
    lp = torch.where(greedy, lp_greedy, lp)
    tok = torch.where(bad, torch.full_like(tok, -1), tok).reshape(logits.shape[:-1])
    if not return_logprobs:
        return tok
    lp = torch.where(bad, torch.full_like(lp, float("nan")), lp).float()
    return tok, lp.reshape(logits.shape[:-1])


def sample_rows(logits: Tensor, temperature=1.0, top_k=0, top_p=1.0, seed: int = 0, stream=None, offset=None,
                return_logprobs: bool = False):
    """One sampled token per row of ``logits`` (R, V) -- or (..., V), flattened -- in one launch
    (``dta_sample_rows``): temperature (``<= 0``: greedy), top-k (``<= 0`` or ``>= V``: off) and top-p
    (``>= 1`` or ``<= 0``: off), each a scalar or a device tensor of R entries, and a uniform drawn by
    Philox4x32-10 from ``(seed, stream[r], offset[r])`` (int64 tensors; default the row index and 0).
    A row's result is a bitwise function of the row, its parameters and that triple: the same in any
    batch, at any row index, from an eager call or a graph replay.

    Returns int64 tokens shaped like ``logits`` without its last dimension, -1 for a row that holds
    a NaN or +inf or is all -inf; with ``return_logprobs`` also the fp32 log-probability of each
    token under the filtered, tempered distribution (greedy: under the plain softmax).

    bf16, fp16 or fp32 logits, any row stride, ``1 <= V <= 2^20``.  CPU tensors, and a library
    without the entry point, run ``sample_rows_reference``."""
    x2 = _sample_rows_2d(logits)
    if x2.device.type != "cuda" or not sample_supported():
        return sample_rows_reference(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs)
    R, V = x2.shape
    dev = x2.device
    T, T_dev = _sample_param(temperature, R, torch.float32, dev, "temperature")
    k, k_dev = _sample_param(top_k, R, torch.int32, dev, "top_k")
    p, p_dev = _sample_param(top_p, R, torch.float32, dev, "top_p")
    strm = _sample_counter(stream, R, dev, "stream")
    off = _sample_counter(offset, R, dev, "offset")
    tokens = torch.empty(R, device=dev, dtype=torch.int64)
    logprobs = torch.empty(R, device=dev, dtype=torch.float32) if return_logprobs else None
    if R > 0:
        k = max(min(k, 2 ** 31 - 1), 0) if k is not None else 0
        a = _lib.SampleRowsArgs(_lib.dtype_code(x2.dtype), R, V, x2.data_ptr(), x2.stride(0),
                                1.0 if T is None else T, k, 1.0 if p is None else p,
                                _lib.ptr(T_dev), _lib.ptr(k_dev), _lib.ptr(p_dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                _lib.ptr(strm), _lib.ptr(off), tokens.data_ptr(), _lib.ptr(logprobs))
        _lib.check(_lib.load().dta_sample_rows(a, _lib.stream_handle(dev)))
    tokens = tokens.reshape(logits.shape[:-1])
    return (tokens, logprobs.reshape(logits.shape[:-1])) if return_logprobs else tokens


# ------------------------------------------------------- sampling penalties ---
# Repetition / frequency / presence penalties, a logit bias and the min-p floor of logits rows, written as
# fp32 rows for ``sample_rows``.  A row is penalised with its sequence's token history plus the drafted
# tokens that precede it in a speculative round, so a round's rows see what the plain loop would have seen.
# The definition is include/diffattn.h's ("Sampling penalties"); ``penalize_rows`` is the HIP kernel,
# ``penalize_rows_reference`` the same definition in torch.
PENALTY_LDS_MAX_V = 40944          # DTA_PENALTY_LDS_MAX_V: up to here the count table is in LDS, no workspace
_PENALTY_WS: Dict[Tuple[torch.device, int], Tensor] = {}


def penalize_rows_supported() -> bool:
    """Whether the loaded library has ``dta_penalize_rows`` (an older build of the same ABI may not)."""
    return _lib.penalty_symbols(_lib.load())


def _penalty_param(v, B: int, device, name: str):
    """A penalty parameter as (scalar, per-sequence fp32 tensor or None)."""
    if isinstance(v, Tensor):
        if v.numel() != B or v.device != device:
            raise ValueError(f"{name} must be a scalar or a tensor of {B} entries on {device}")
        return None, v.reshape(B).to(torch.float32).contiguous()
    v = float(v)
    if v != v:
        raise ValueError(f"{name} is NaN")
    return v, None


def _penalty_check(logits, hist, hlen, gen_start, draft, dcnt, repetition, presence, frequency, floor_gap, bias,
                   rows_per_seq, out):
    """The shapes and values both implementations insist on; returns (x2, B, Tn, K, the four parameters as
    (scalar, tensor) pairs, bias as (B or 1, V) or None)."""
    x2 = _sample_rows_2d(logits)
    R, V = x2.shape
    dev = x2.device
    Tn = int(rows_per_seq)
    if hist.dim() != 2 or hist.shape[1] < 1 or Tn < 1:
        raise ValueError("hist must be (B, cap) with cap >= 1, and rows_per_seq >= 1")
    B, cap = hist.shape
    if R != B * Tn:
        raise ValueError(f"logits has {R} rows, hist {B} sequences of rows_per_seq {Tn} rows each")
    if cap > 1 << 30:
        raise ValueError(f"cap {cap} is above 2^30")
    if (draft is None) != (dcnt is None):
        raise ValueError("draft and dcnt come together")
    K = 0
    ints = [("hist", hist, (B, cap)), ("hlen", hlen, (B,))]
    if gen_start is not None:
        ints.append(("gen_start", gen_start, (B,)))
    if draft is not None:
        if draft.dim() != 2 or draft.shape[1] > SPEC_MAX_K:
            raise ValueError(f"draft must be (B, K) with K <= {SPEC_MAX_K}")
        K = draft.shape[1]
        ints += [("draft", draft, (B, K)), ("dcnt", dcnt, (B,))]
    for name, t, shape in ints:
        if not isinstance(t, Tensor) or t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} must be an int32 {shape} tensor on {dev}")
        if t.dim() == 1 and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.dim() == 2 and ((t.stride(1) != 1 and t.shape[1] > 1) or (B > 1 and t.stride(0) < t.shape[1])):
            raise ValueError(f"{name} must have contiguous rows")
    theta = _penalty_param(repetition, B, dev, "repetition")
    if theta[0] is not None and theta[0] <= 0:
        raise ValueError(f"repetition {theta[0]} must be positive")
    pres = _penalty_param(presence, B, dev, "presence")
    freq = _penalty_param(frequency, B, dev, "frequency")
    gap = _penalty_param(0.0 if floor_gap is None else floor_gap, B, dev, "floor_gap")
    if bias is not None:
        if not isinstance(bias, Tensor) or bias.dtype != torch.float32 or bias.device != dev or \
                tuple(bias.shape) not in ((V,), (1, V), (B, V)) or (V > 1 and bias.stride(-1) != 1):
            raise ValueError(f"bias must be an fp32 ({V},) or ({B}, {V}) tensor on {dev} with contiguous rows")
        bias = bias.reshape(-1, V)
    if out is not None:
        if not isinstance(out, Tensor) or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (R, V) \
                or (V > 1 and out.stride(1) != 1) or (R > 1 and out.stride(0) < V):
            raise ValueError(f"out must be an fp32 ({R}, {V}) tensor on {dev} with contiguous rows that do not overlap")
    return x2, B, Tn, K, theta, pres, freq, gap, bias


def penalize_rows_reference(logits: Tensor, hist: Tensor, hlen: Tensor, gen_start: Optional[Tensor] = None,
                            draft: Optional[Tensor] = None, dcnt: Optional[Tensor] = None, repetition=1.0,
                            presence=0.0, frequency=0.0, floor_gap=None, bias: Optional[Tensor] = None,
                            rows_per_seq: int = 1, out: Optional[Tensor] = None) -> Tensor:
    """``penalize_rows`` in torch fp32 elementwise ops, on the tensors' device: include/diffattn.h's definition,
    one rounding per operation.  Run on CPU tensors it equals the kernel bit for bit (the GPU tests hold the
    kernel to that run; the payload of a NaN that the arithmetic itself makes, inf - inf, is the one thing left
    open); run on the GPU it is torch's device arithmetic, which has not been held to the kernel's last bit.
    The tests' oracle, and what ``penalize_rows`` runs on CPU tensors and on a library without
    ``dta_penalize_rows``."""
    x2, B, Tn, K, theta, pres, freq, gap, bias = _penalty_check(logits, hist, hlen, gen_start, draft, dcnt, repetition,
                                                                presence, frequency, floor_gap, bias, rows_per_seq, out)
    R, V = x2.shape
    dev = x2.device
    cap = hist.shape[1]
    rows = lambda sv: (sv[1] if sv[1] is not None else torch.full((B,), sv[0], dtype=torch.float32, device=dev)
                       ).repeat_interleave(Tn)[:, None]                                   # noqa: E731
    theta, pres, freq, gap = rows(theta), rows(pres), rows(freq), rows(gap)
    # the context: counts of the history from gen_start on, the seen flag of all of it, the draft prefix per row
    L = hlen.long().clamp(0, cap)
    g = (gen_start.long() if gen_start is not None else torch.zeros_like(L)).clamp(min=0).minimum(L)
    t = torch.arange(cap, device=dev)[None, :]
    h = hist.long()
    ok = (t < L[:, None]) & (h >= 0) & (h < V)
    col = torch.where(ok, h, V)                                                           # column V: ignored
    seen = torch.zeros(B, V + 1, dtype=torch.int64, device=dev).scatter_add_(1, col, ok.long())
    cnt = torch.zeros(B, V + 1, dtype=torch.int64, device=dev).scatter_add_(1, col, (ok & (t >= g[:, None])).long())
    seen, cnt = seen.repeat_interleave(Tn, dim=0), cnt.repeat_interleave(Tn, dim=0)
    if draft is not None and K > 0:
        j = torch.arange(Tn, device=dev).repeat(B)
        e = torch.minimum(j, dcnt.long().clamp(0, K).repeat_interleave(Tn))
        dr = draft.long().repeat_interleave(Tn, dim=0)
        ok = (torch.arange(K, device=dev)[None, :] < e[:, None]) & (dr >= 0) & (dr < V)
        add = torch.zeros(R, V + 1, dtype=torch.int64, device=dev).scatter_add_(1, torch.where(ok, dr, V), ok.long())
        seen, cnt = seen + add, cnt + add
    seen, cnt = seen[:, :V] > 0, cnt[:, :V]
    x0 = x2.float()
    nan = torch.isnan(x0)
    ninf = torch.full_like(x0, float("-inf"))
    x = x0
    on = ~torch.isnan(theta) & (theta != 1)
    x = torch.where(seen & on, torch.where(x > 0, x / theta, x * theta), x)
    on = ~torch.isnan(freq) & ~torch.isnan(pres)
    x = torch.where((cnt > 0) & on, (x - freq * cnt.float()) - pres, x)
    if bias is not None:
        x = x + (bias if bias.shape[0] == 1 else bias.repeat_interleave(Tn, dim=0))
    m = torch.where(torch.isnan(x), ninf, x).max(dim=1, keepdim=True).values
    on = torch.isfinite(gap) & (gap < 0) & torch.isfinite(m)
    x = torch.where(on & ~torch.isnan(x) & ~(x >= m + gap), ninf, x)       # a NaN the arithmetic made stays one
    x = torch.where(nan, x0, x)
    if out is None:
        return x.reshape(logits.shape)
    out.copy_(x)
    return out


def penalize_rows(logits: Tensor, hist: Tensor, hlen: Tensor, gen_start: Optional[Tensor] = None,
                  draft: Optional[Tensor] = None, dcnt: Optional[Tensor] = None, repetition=1.0, presence=0.0,
                  frequency=0.0, floor_gap=None, bias: Optional[Tensor] = None, rows_per_seq: int = 1,
                  out: Optional[Tensor] = None) -> Tensor:
    """Penalised fp32 logits of B * ``rows_per_seq`` rows in one launch (``dta_penalize_rows``).  ``logits``
    (B * rows_per_seq, V) -- or (..., V), flattened -- bf16, fp16 or fp32, any row stride; row ``j`` of sequence
    ``b`` is penalised with ``hist[b, :hlen[b]]`` (int32 (B, cap) and (B,)) followed by the first
    ``min(j, dcnt[b])`` tokens of ``draft[b]`` (int32 (B, K), K <= 7; optional).  ``gen_start`` int32 (B,): the
    prompt lengths (None: 0) -- frequency and presence count from there on, repetition sees everything.
    ``repetition`` (1: off; > 0), ``presence``, ``frequency``, ``floor_gap`` (``T * ln(min_p)`` as fp32; None or
    ``>= 0``: off): each a scalar or a device tensor of B entries.  ``bias``: fp32 (V,) or (B, V), added after
    the penalties; ``-inf`` bans a token.  A row's output is a bitwise function of the row, its sequence's state
    and its parameters.  Returns fp32 shaped like ``logits`` (or ``out``, fp32 (R, V), rows of any stride).

    ``V`` above ``PENALTY_LDS_MAX_V`` counts in a workspace kept per (device, size), so that a graph-captured
    caller holds it by address; the buffers (4 R V bytes each) are kept for the life of the process, one per
    distinct size -- eager speculative rounds of varying width make up to K + 1 of them.  CPU tensors, and a
    library without the entry point, run ``penalize_rows_reference``."""
    args = (logits, hist, hlen, gen_start, draft, dcnt, repetition, presence, frequency, floor_gap, bias, rows_per_seq, out)
    if not isinstance(logits, Tensor) or logits.device.type != "cuda" or not penalize_rows_supported():
        return penalize_rows_reference(*args)
    x2, B, Tn, K, theta, pres, freq, gap, bias = _penalty_check(*args)
    R, V = x2.shape
    dev = x2.device
    res = torch.empty(R, V, device=dev, dtype=torch.float32) if out is None else out
    if R > 0:
        lib = _lib.load()
        need = lib.dta_penalize_rows_workspace_bytes(R, V)
        ws = None
        if need:
            ws = _PENALTY_WS.get((dev, need))
            if ws is None:
                ws = _PENALTY_WS[(dev, need)] = torch.empty(need, device=dev, dtype=torch.uint8)
        row = lambda t, n: t.stride(0) if t.shape[0] > 1 else n                           # noqa: E731
        sc = lambda sv, default: default if sv[0] is None else sv[0]                      # noqa: E731
        a = _lib.PenalizeRowsArgs(_lib.dtype_code(x2.dtype), B, Tn, V, hist.shape[1], K,
                                  x2.data_ptr(), row(x2, V), res.data_ptr(), row(res, V),
                                  hist.data_ptr(), row(hist, hist.shape[1]), hlen.data_ptr(), _lib.ptr(gen_start),
                                  _lib.ptr(draft), row(draft, K) if draft is not None else 0, _lib.ptr(dcnt),
                                  sc(theta, 1.0), sc(freq, 0.0), sc(pres, 0.0), sc(gap, 0.0),
                                  _lib.ptr(theta[1]), _lib.ptr(freq[1]), _lib.ptr(pres[1]), _lib.ptr(gap[1]),
                                  _lib.ptr(bias), 0 if bias is None or bias.shape[0] == 1 else bias.stride(0),
                                  _lib.ptr(ws), need)
        _lib.check(lib.dta_penalize_rows(a, _lib.stream_handle(dev)))
    return res.reshape(logits.shape) if out is None else out


# ------------------------------------------------------ speculative decoding ---
# One round of prompt-lookup speculative decoding on the device: which of the round's sampled rows are
# emitted, the append to the sequence's history and the next draft by n-gram lookup.  The definition is
# include/diffattn.h's ("Speculative decoding"); ``spec_accept_draft`` is the HIP kernel,
# ``spec_accept_draft_reference`` the same definition in torch.  Both update the state in place.
SPEC_MAX_K = 7
SPEC_MAX_NGRAM = 8


def spec_supported() -> bool:
    """Whether the loaded library has ``dta_spec_accept_draft`` (an older build of the same ABI may not)."""
    return _lib.spec_symbols(_lib.load())


def _spec_check(hist, hlen, remaining, draft, dcnt, tok, result, k, ngram_min, ngram_max, t_cap):
    """The shapes and values both implementations insist on; returns (B, cap, Tn, tok as (B, Tn) or None)."""
    k, ngram_min, ngram_max, t_cap = int(k), int(ngram_min), int(ngram_max), int(t_cap)
    if not 1 <= k <= SPEC_MAX_K:
        raise ValueError(f"k {k} outside 1 .. {SPEC_MAX_K}")
    if not (0 <= ngram_min <= ngram_max and 1 <= ngram_max <= SPEC_MAX_NGRAM):
        raise ValueError(f"need 0 <= ngram_min {ngram_min} <= ngram_max {ngram_max}, 1 <= ngram_max <= {SPEC_MAX_NGRAM}")
    if hist.dim() != 2 or hist.shape[1] < 1 or t_cap < 1:
        raise ValueError("hist must be (B, cap) with cap >= 1, and t_cap >= 1")
    B, cap = hist.shape
    Tn = 0
    if tok is not None:
        if tok.dim() != 2 or tok.shape[0] != B or tok.dtype != torch.int64 or tok.device != hist.device:
            raise ValueError(f"tok must be an int64 (B, Tn) tensor on {hist.device}")
        Tn = tok.shape[1]
        if Tn > k + 1:
            raise ValueError(f"tok has {Tn} columns, a round has at most k + 1 = {k + 1} rows")
    for name, t, shape in (("hist", hist, (B, cap)), ("hlen", hlen, (B,)), ("remaining", remaining, (B,)),
                           ("draft", draft, (B, k)), ("dcnt", dcnt, (B,)), ("result", result, (B, 2))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != hist.device:
            raise ValueError(f"{name} must be an int32 {shape} tensor on {hist.device}")
        if (t.stride(-1) != 1 and t.shape[-1] > 1) or (t.dim() == 2 and B > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"{name} must have contiguous rows that do not overlap: it is updated in place")
    for name, t in (("hlen", hlen), ("remaining", remaining), ("dcnt", dcnt), ("result", result)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return B, cap, Tn


def spec_accept_draft_reference(hist: Tensor, hlen: Tensor, remaining: Tensor, draft: Tensor, dcnt: Tensor,
                                tok: Optional[Tensor], eos_id: int = -1, k: int = 4, ngram_min: int = 1,
                                ngram_max: int = 3, t_cap: int = 1 << 30, result: Optional[Tensor] = None) -> Tensor:
    """``spec_accept_draft`` in torch and Python, on the tensors' device: include/diffattn.h's definition
    a row at a time, the lookup vectorised over the ends.  The tests' oracle, and what
    ``spec_accept_draft`` runs on CPU tensors and on a library without the entry point."""
    if result is None:
        result = torch.zeros(hist.shape[0], 2, dtype=torch.int32, device=hist.device)
    B, cap, Tn = _spec_check(hist, hlen, remaining, draft, dcnt, tok, result, k, ngram_min, ngram_max, t_cap)
    k, ngram_min, ngram_max, t_cap, eos_id = int(k), int(ngram_min), int(ngram_max), int(t_cap), int(eos_id)
    lens, rems, dcs = hlen.tolist(), remaining.tolist(), dcnt.tolist()
    toks = tok.tolist() if Tn else [[] for _ in range(B)]
    for b in range(B):
        rem = rems[b]
        if rem <= 0:
            result[b, 0], result[b, 1] = 0, 0
            continue
        L0 = min(max(lens[b], 0), cap)
        dc = min(max(dcs[b], 0), min(k, max(Tn - 1, 0)))
        t, d = toks[b], draft[b, :dc].tolist()
        a = 0
        while a < dc and t[a] == d[a]:
            a += 1
        m = min(a + 1, rem, Tn, cap - L0)
        stop = False
        for j in range(m):
            if t[j] < 0 or t[j] == eos_id:
                m, stop = j + 1, True
                break
        rem = 0 if stop else rem - m
        if m:
            hist[b, L0:L0 + m] = torch.tensor(t[:m], dtype=torch.int64, device=hist.device).to(torch.int32)
        L = L0 + m
        nd = 0
        if ngram_min >= 1 and rem > 1 and L > ngram_min:
            h = hist[b, :L].long()
            e = torch.arange(ngram_min - 1, L - 1, device=h.device)
            same = torch.ones_like(e, dtype=torch.bool)
            mu = torch.zeros_like(e)
            for n in range(min(ngram_max, L - 1)):               # mu(e) <= e + 1 <= L - 1
                ok = e - n >= 0
                same = same & ok & (h[(e - n).clamp(min=0)] == h[L - 1 - n])
                mu = mu + same
            key = torch.where(mu >= ngram_min, (mu << 32) | e, torch.zeros_like(e))
            best = int(key.max())
            if best:
                end = best & 0xFFFFFFFF
                nd = max(min(k, L - 1 - end, rem - 1, t_cap - L), 0)
                if nd:
                    draft[b, :nd] = hist[b, end + 1:end + 1 + nd]
        hlen[b], remaining[b], dcnt[b] = L, rem, nd
        result[b, 0], result[b, 1] = m, nd
    return result


def spec_accept_draft(hist: Tensor, hlen: Tensor, remaining: Tensor, draft: Tensor, dcnt: Tensor,
                      tok: Optional[Tensor], eos_id: int = -1, k: int = 4, ngram_min: int = 1, ngram_max: int = 3,
                      t_cap: int = 1 << 30, result: Optional[Tensor] = None) -> Tensor:
    """One round of speculative decoding for B sequences in one launch (``dta_spec_accept_draft``), on the
    loop's device state, updated in place: ``hist`` int32 (B, cap) token histories of ``hlen`` tokens each
    (the last one pending), ``remaining`` tokens still owed (``<= 0``: finished, the row is not touched),
    ``draft`` int32 (B, k) and its lengths ``dcnt``.  ``tok`` int64 (B, Tn), ``Tn <= k + 1``: the samples of
    the round's logits rows (row 0 after the pending token, row j after ``draft[j - 1]``), any row stride;
    None: no rows, only a draft.  The leading drafts that equal their samples are accepted, one more sample
    is emitted (``eos_id`` or a negative token ends the sequence), the emitted tokens join ``hist``, and the
    next draft is the continuation of the longest, then latest, earlier occurrence of the history's last
    ``ngram_min .. ngram_max`` tokens, at most ``min(k, remaining - 1, t_cap - hlen)`` long
    (``ngram_min = 0``: no lookup, the next ``dcnt`` is 0).  Returns ``result`` int32 (B, 2): (tokens
    emitted m, next dcnt) -- the cache keeps its old length + m rows.

    CPU tensors, and a library without the entry point, run ``spec_accept_draft_reference``."""
    if hist.device.type != "cuda" or not spec_supported():
        return spec_accept_draft_reference(hist, hlen, remaining, draft, dcnt, tok, eos_id, k, ngram_min, ngram_max,
                                           t_cap, result)
    if result is None:
        result = torch.empty(hist.shape[0], 2, dtype=torch.int32, device=hist.device)
    B, cap, Tn = _spec_check(hist, hlen, remaining, draft, dcnt, tok, result, k, ngram_min, ngram_max, t_cap)
    if cap > 1 << 30:
        raise ValueError(f"cap {cap} is above 2^30")
    if Tn and ((tok.stride(1) != 1 and Tn > 1) or (tok.stride(0) < Tn and B > 1)):
        tok = tok.contiguous()
    if B > 0:
        row = lambda t, n: t.stride(0) if B > 1 else n                                # noqa: E731
        a = _lib.SpecAcceptDraftArgs(B, Tn, int(k), cap, min(int(t_cap), 1 << 30), int(ngram_min), int(ngram_max),
                                     max(min(int(eos_id), 2 ** 31 - 1), -1), row(hist, cap), row(draft, int(k)),
                                     row(tok, Tn) if Tn else 0, hist.data_ptr(), hlen.data_ptr(), remaining.data_ptr(),
                                     draft.data_ptr(), dcnt.data_ptr(), tok.data_ptr() if Tn else None,
                                     result.data_ptr())
        _lib.check(_lib.load().dta_spec_accept_draft(a, _lib.stream_handle(hist.device)))
    return result


# The glue of a fixed-shape round (always k + 1 rows per sequence), so that no host value shapes it and it can
# be captured once and replayed (``kv_cache.SpecRound``): the round's tokens, counts and sampler offsets from
# the state above, and the cache lengths after the accept.  include/diffattn.h ("A fixed-shape speculative
# round") is the definition; the ``*_reference`` functions are the same definition in torch.
def spec_round_supported() -> bool:
    """Whether the loaded library has ``dta_spec_feed_rows`` and ``dta_spec_commit_lengths`` (an older build
    of the same ABI may not)."""
    return _lib.spec_round_symbols(_lib.load())


def _need_spec_round(device) -> None:
    if not spec_round_supported():
        raise RuntimeError("this libdiffattn.so exports no dta_spec_feed_rows / dta_spec_commit_lengths "
                           f"(ops.spec_round_supported); there is no fallback on {device}")


def _spec_feed_check(hist, hlen, remaining, draft, dcnt, k, vocab, total, idx_out, counts_out, offset_out):
    """The shapes and values both implementations insist on; returns (B, cap, idx_out, counts_out, offset_out),
    the outputs allocated where they were not given."""
    k, vocab, total = int(k), int(vocab), int(total)
    if not 1 <= k <= SPEC_MAX_K:
        raise ValueError(f"k {k} outside 1 .. {SPEC_MAX_K}")
    if vocab < 1 or total < 0 or vocab > 2 ** 31 - 1 or total > 2 ** 31 - 1:
        raise ValueError(f"need 1 <= vocab {vocab} and 0 <= total {total}, both int32")
    if hist.dim() != 2 or hist.shape[1] < 1:
        raise ValueError("hist must be (B, cap) with cap >= 1")
    B, cap = hist.shape
    dev = hist.device
    if idx_out is None:
        idx_out = torch.empty(B, k + 1, dtype=torch.int64, device=dev)
    if counts_out is None:
        counts_out = torch.empty(B, dtype=torch.int32, device=dev)
    if offset_out is None:
        offset_out = torch.empty(B, k + 1, dtype=torch.int64, device=dev)
    for name, t, shape, dt in (("hist", hist, (B, cap), torch.int32), ("hlen", hlen, (B,), torch.int32),
                               ("remaining", remaining, (B,), torch.int32), ("draft", draft, (B, k), torch.int32),
                               ("dcnt", dcnt, (B,), torch.int32), ("idx_out", idx_out, (B, k + 1), torch.int64),
                               ("counts_out", counts_out, (B,), torch.int32),
                               ("offset_out", offset_out, (B, k + 1), torch.int64)):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} must be a {dt} {shape} tensor on {dev}")
        if (t.stride(-1) != 1 and t.shape[-1] > 1) or (t.dim() == 2 and B > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"{name} must have contiguous rows that do not overlap")
    for name, t in (("hlen", hlen), ("remaining", remaining), ("dcnt", dcnt), ("counts_out", counts_out)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return B, cap, idx_out, counts_out, offset_out


def spec_feed_rows_reference(hist: Tensor, hlen: Tensor, remaining: Tensor, draft: Tensor, dcnt: Tensor, k: int,
                             vocab: int, total: int, idx_out: Optional[Tensor] = None,
                             counts_out: Optional[Tensor] = None, offset_out: Optional[Tensor] = None):
    """``spec_feed_rows`` in torch, on the tensors' device: include/diffattn.h's definition over the whole
    batch.  The tests' oracle, and what ``spec_feed_rows`` runs on CPU tensors."""
    B, cap, idx_out, counts_out, offset_out = _spec_feed_check(hist, hlen, remaining, draft, dcnt, k, vocab, total,
                                                               idx_out, counts_out, offset_out)
    k, vocab, total = int(k), int(vocab), int(total)
    L = hlen.clamp(0, cap)
    live = (remaining > 0) & (L >= 1)
    zero = torch.zeros_like(L)
    d = torch.where(live, dcnt.clamp(0, k), zero)
    counts_out.copy_(torch.where(live, d + 1, zero))
    pending = hist.gather(1, (L.long() - 1).clamp_(min=0)[:, None])[:, 0].clamp(0, vocab - 1)
    idx_out[:, 0] = torch.where(live, pending, zero).long()
    j = torch.arange(1, k + 1, device=hist.device)
    idx_out[:, 1:] = torch.where(j[None, :] <= d[:, None], draft.clamp(0, vocab - 1), 0).long()
    offset_out.copy_((total - remaining.long())[:, None] + torch.arange(k + 1, device=hist.device)[None, :])
    return idx_out, counts_out, offset_out


def spec_feed_rows(hist: Tensor, hlen: Tensor, remaining: Tensor, draft: Tensor, dcnt: Tensor, k: int, vocab: int,
                   total: int, idx_out: Optional[Tensor] = None, counts_out: Optional[Tensor] = None,
                   offset_out: Optional[Tensor] = None):
    """The model inputs of one fixed-shape round of B sequences in one launch (``dta_spec_feed_rows``), from
    the state ``spec_accept_draft`` keeps, none of it read on the host: ``idx_out`` int64 (B, k + 1), the
    pending token ``hist[b, hlen[b] - 1]`` followed by the ``dcnt[b]`` drafted ones and zeros, each clamped
    into ``[0, vocab - 1]``; ``counts_out`` int32 (B,), ``dcnt[b] + 1`` real rows, 0 for a sequence with
    ``remaining[b] <= 0`` (or no history); ``offset_out`` int64 (B, k + 1), ``total - remaining[b] + j``:
    the ``sample_rows`` offset of the plain loop at row j.  Every entry of the three is written.  The
    outputs may be given (any row stride; what a captured graph holds by address).  Returns
    (idx_out, counts_out, offset_out).

    CPU tensors run ``spec_feed_rows_reference``; on the GPU a library without the entry point is a
    ``RuntimeError``."""
    if hist.device.type != "cuda":
        return spec_feed_rows_reference(hist, hlen, remaining, draft, dcnt, k, vocab, total, idx_out, counts_out,
                                        offset_out)
    _need_spec_round(hist.device)
    B, cap, idx_out, counts_out, offset_out = _spec_feed_check(hist, hlen, remaining, draft, dcnt, k, vocab, total,
                                                               idx_out, counts_out, offset_out)
    if cap > 1 << 30:
        raise ValueError(f"cap {cap} is above 2^30")
    if B > 0:
        row = lambda t, n: t.stride(0) if B > 1 else n                                # noqa: E731
        a = _lib.SpecFeedRowsArgs(B, int(k), cap, int(vocab), int(total), row(hist, cap), row(draft, int(k)),
                                  row(idx_out, int(k) + 1), row(offset_out, int(k) + 1), hist.data_ptr(),
                                  hlen.data_ptr(), remaining.data_ptr(), draft.data_ptr(), dcnt.data_ptr(),
                                  idx_out.data_ptr(), counts_out.data_ptr(), offset_out.data_ptr())
        _lib.check(_lib.load().dta_spec_feed_rows(a, _lib.stream_handle(hist.device)))
    return idx_out, counts_out, offset_out


def _spec_commit_check(lengths, result, k, t_cap, slots):
    k, t_cap = int(k), int(t_cap)
    if not 1 <= k <= SPEC_MAX_K:
        raise ValueError(f"k {k} outside 1 .. {SPEC_MAX_K}")
    if t_cap < 1:
        raise ValueError("t_cap must be >= 1")
    if lengths.dim() != 1 or lengths.shape[0] < 1 or lengths.dtype != torch.int32 or not lengths.is_contiguous():
        raise ValueError("lengths must be a contiguous int32 (n_slots,) tensor, n_slots >= 1")
    dev = lengths.device
    if result.dim() != 2 or result.shape[1] != 2 or result.dtype != torch.int32 or result.device != dev \
            or not result.is_contiguous():
        raise ValueError(f"result must be a contiguous int32 (B, 2) tensor on {dev}")
    B = result.shape[0]
    if slots is None:
        if B > lengths.shape[0]:
            raise ValueError(f"{B} sequences for {lengths.shape[0]} lengths")
    elif tuple(slots.shape) != (B,) or slots.dtype != torch.int64 or slots.device != dev or not slots.is_contiguous():
        raise ValueError(f"slots must be a contiguous int64 ({B},) tensor on {dev}")
    return B


def spec_commit_lengths_reference(lengths: Tensor, result: Tensor, k: int, t_cap: int,
                                  slots: Optional[Tensor] = None) -> Tensor:
    """``spec_commit_lengths`` in torch, on the tensors' device, in place.  The tests' oracle, and what
    ``spec_commit_lengths`` runs on CPU tensors."""
    B = _spec_commit_check(lengths, result, k, t_cap, slots)
    if B == 0:
        return lengths
    s = torch.arange(B, device=lengths.device) if slots is None else slots.clamp(0, lengths.shape[0] - 1)
    new = (lengths[s].long() + result[:, 0].clamp(0, int(k) + 1).long()).clamp_(max=int(t_cap))
    lengths[s] = new.to(torch.int32)
    return lengths


def spec_commit_lengths(lengths: Tensor, result: Tensor, k: int, t_cap: int, slots: Optional[Tensor] = None) -> Tensor:
    """The device half of a round's roll-back, in one launch (``dta_spec_commit_lengths``): the round's model
    step leaves the cache's ``lengths`` int32 (n_slots,) alone, and this adds what the round emitted,
    ``lengths[s] = min(lengths[s] + clamp(result[b, 0], 0, k + 1), t_cap)`` with ``s = slots[b]`` (int64 (B,),
    distinct, clamped into the tensor; None: ``s = b``) and ``result`` the (B, 2) output of
    ``spec_accept_draft``.  An entry no sequence names is not touched.  In place; returns ``lengths``.

    CPU tensors run ``spec_commit_lengths_reference``; on the GPU a library without the entry point is a
    ``RuntimeError``."""
    if lengths.device.type != "cuda":
        return spec_commit_lengths_reference(lengths, result, k, t_cap, slots)
    _need_spec_round(lengths.device)
    B = _spec_commit_check(lengths, result, k, t_cap, slots)
    if B > 0:
        a = _lib.SpecCommitLengthsArgs(B, int(k), min(int(t_cap), 1 << 30), lengths.shape[0], lengths.data_ptr(),
                                       result.data_ptr(), _lib.ptr(slots))
        _lib.check(_lib.load().dta_spec_commit_lengths(a, _lib.stream_handle(lengths.device)))
    return lengths


# ------------------------------------------------------ shared-prefix decode ---
# The one-row paged decode for a batch in which groups of sequences have the same pool pages under
# their first rows (``PagedKVCache.fork``, ``generate_paged(n_samples=k)``): a group pass reads the
# shared rows once per group, the one-row pass reads what is left (include/diffattn.h "Shared-prefix
# decode").  Bitwise ``diff_attention_decode_paged(_fp8)`` on the same inputs.
SHARED_GROUP_MAX = 8


class SharedDecodePlan:
    """The groups of one decode step on the device: ``members`` int32 (n_groups, 8), batch indices
    padded with -1; ``rows`` int32 (n_groups,), the rows every member of a group reaches through
    the same pages.  Built once per step (``shared_decode_plan``) and used by every layer."""

    def __init__(self, B: int, groups, shared_rows, members: Optional[Tensor], rows: Optional[Tensor]):
        self.B = B
        self.groups = groups
        self.shared_rows = shared_rows
        self.n_groups = len(groups)
        self.members = members
        self.rows = rows


def shared_decode_plan(groups, shared_rows, B: int, device) -> SharedDecodePlan:
    """Validate a step's groups on the host and upload them once.  ``groups``: sequences of 2 .. 8
    distinct batch indices in [0, B), no index in two groups; ``shared_rows[g] >= 0``: cache rows
    0 .. shared_rows[g]-1 are the same pool pages in the block-table row of every member of group
    g (the caller's promise: the kernels keep every access in range whatever the plan says, but
    only a true plan gives the paged op's result)."""
    groups = [tuple(int(b) for b in g) for g in groups]
    shared_rows = [int(r) for r in shared_rows]
    if len(groups) != len(shared_rows):
        raise ValueError(f"{len(groups)} groups, {len(shared_rows)} shared row counts")
    seen = set()
    for g, r in zip(groups, shared_rows):
        if not 2 <= len(g) <= SHARED_GROUP_MAX:
            raise ValueError(f"a group has {len(g)} members, outside 2 .. {SHARED_GROUP_MAX}")
        for b in g:
            if not 0 <= b < B:
                raise ValueError(f"member {b} outside the batch of {B}")
            if b in seen:
                raise ValueError(f"sequence {b} is named twice")
            seen.add(b)
        if r < 0:
            raise ValueError(f"shared rows {r} < 0")
    if not groups:
        return SharedDecodePlan(B, groups, shared_rows, None, None)
    pad = [list(g) + [-1] * (SHARED_GROUP_MAX - len(g)) for g in groups]
    both = torch.tensor([x for g in pad for x in g] + shared_rows, dtype=torch.int32).to(device)    # one copy
    n = len(groups) * SHARED_GROUP_MAX
    return SharedDecodePlan(B, groups, shared_rows, both[:n].view(-1, SHARED_GROUP_MAX), both[n:])


def decode_shared_supported(dtype: torch.dtype, hs: int, N: int, dv: int, fp8: bool = False) -> bool:
    """Whether ``diff_attention_decode_paged_shared`` (``fp8``: ``..._fp8``) has a kernel plan
    (dta_decode_shared_supported): the split-key shapes of ``decode_rows_supported``.  False on a
    library without the entry points."""
    lib = _lib.load()
    return _lib.shared_symbols(lib) and bool(
        lib.dta_decode_shared_supported(_lib.dtype_code(dtype), hs, N, dv, int(bool(fp8))))


def _shared_plan(lib, plan, B: int, q: Tensor) -> None:
    if not _lib.shared_symbols(lib):
        raise RuntimeError("this libdiffattn.so has no shared-prefix decode entry points (decode_shared_supported)")
    if not isinstance(plan, SharedDecodePlan):
        raise RuntimeError("plan must be a SharedDecodePlan (shared_decode_plan)")
    if plan.B != B:
        raise RuntimeError(f"the plan was made for a batch of {plan.B}, q holds {B}")
    if plan.n_groups and plan.members.device != q.device:
        raise RuntimeError(f"the plan lives on {plan.members.device}, q on {q.device}")


def diff_attention_decode_paged_shared(q: Tensor, k_pool: Tensor, v_pool: Tensor, coef: Tensor, block_table: Tensor,
                                       lengths: Tensor, plan: SharedDecodePlan,
                                       max_length: Optional[int] = None) -> Tensor:
    """``diff_attention_decode_paged`` under a shared-prefix plan: the rows a group shares are
    loaded once per group.  Arguments, checks, clamps and result as the paged op's; bitwise equal
    to it where the plan is true.  No fallback: raises without a plan, without a kernel plan for
    the shape (``decode_shared_supported``) or on a library without the entry points."""
    lib = _lib.load()
    _require_gpu(q, k_pool, v_pool, coef)
    B, H, N, hs = q.shape
    _shared_plan(lib, plan, B, q)
    return _decode_paged(lib, q, k_pool, v_pool, None, coef, block_table, lengths, max_length, plan)


def diff_attention_decode_paged_shared_fp8(q: Tensor, k_pool_u8: Tensor, v_pool_u8: Tensor, scale_pool: Tensor,
                                           coef: Tensor, block_table: Tensor, lengths: Tensor,
                                           plan: SharedDecodePlan, max_length: Optional[int] = None) -> Tensor:
    """``diff_attention_decode_paged_fp8`` under a shared-prefix plan (bytes and scales of the
    shared rows loaded once per group); otherwise as ``diff_attention_decode_paged_shared``."""
    lib = _lib.load()
    _require_gpu(q, k_pool_u8, v_pool_u8, scale_pool, coef)
    B, H, N, hs = q.shape
    _shared_plan(lib, plan, B, q)
    return _decode_paged(lib, q, k_pool_u8, v_pool_u8, scale_pool, coef, block_table, lengths, max_length, plan)
