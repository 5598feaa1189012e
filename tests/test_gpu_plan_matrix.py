"""Parity for every attention plan the dispatcher can pick, generated instead of hand-picked.

``csrc/capi.hip`` and ``csrc/attn_kernels.h`` select a kernel instantiation on the dtype, the
``DTA_FOR_CONFIGS`` entry (hs, N, dv), dropout on / off, the backward branch-group caps and on
whether the ``lse_c`` and ``dv_f32`` workspaces are passed.  The other GPU modules cover those axes
one at a time; this one runs their cross product (A), the dropout combinations the matrix does not
reach (B), the coefficient scale with the error taken per branch (C) and zero-sized calls on
poisoned memory (D).  ``tests/test_plan_inventory_cpu.py`` pins which plans are native.

Everything is compared with the fp64 oracle of the other modules (``_oracle_core``,
``_oracle_dropped`` with the numpy restatement of the kernels' dropout hash) on inputs quantised to
the kernel dtype, at the project's bars ``TOL``.  Every case is B = 2, H = 2 (H = 1 at head size
256) and T = 70 unless it says otherwise: a ragged last tile and more than one key tile in every
plan.
"""
import contextlib
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from _poison import poisoned_allocations
from conftest import rel_err
from oracle import diffattn_oracle as orc
from test_gpu_dropout import _oracle_dropped, drop_masks
from test_gpu_parity import DEV, TOL, _oracle_core

from differential_transformer_replication_amd import _lib, ops, packing

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
T0 = 70
SEED = 0x1234_5678_9ABC + T0


def _f32(p):
    """``p`` as the C ABI sees it (dta_attn_*_args.dropout_p is a float)."""
    return float(np.float32(p))


# ---- one problem: inputs, and the oracle's outputs and gradients --------------------------
@functools.lru_cache(maxsize=4)
def _problem(dtype, H, N, hs, T, rope, dv, p, seed, coef_rows=None, B=2):
    """Inputs quantised to ``dtype`` and the fp64 reference forward and backward, computed once
    for the cases that share them (caps, workspaces and storage types change the kernels, not
    the problem).  ``coef_rows``: the coefficients as a tuple of rows, else random with c_0 = 1."""
    freqs_c = orc.precompute_freqs_cis(hs, max(T, 8)) if rope else None
    masks = None
    if p:
        masks = drop_masks(seed, p, B, H, N, T)
    elif dv != 2 * hs:
        masks = torch.ones(B, H, N, 1, 1, dtype=torch.float64)
    for draw in range(32):
        g = torch.Generator().manual_seed(1000 * H + 100 * N + hs + T + dv + 7919 * draw)
        qkv = torch.randn(B, T, ops.packed_width(H, N, hs, dv), generator=g).to(dtype)
        coef = torch.randn(H, N, generator=g) * 0.5
        coef[:, 0] = 1.0
        if coef_rows is not None:
            coef = torch.tensor(coef_rows, dtype=torch.float32)
        do = torch.randn(B, T, H * dv, generator=g).to(dtype)
        x64 = qkv.double().requires_grad_(True)
        c64 = coef.double().clone().requires_grad_(True)
        if masks is None:
            ref = _oracle_core(x64, c64, H, N, hs, freqs_c)
        else:
            ref = _oracle_dropped(x64, c64, H, N, hs, dv, masks, freqs_c)
        ref.backward(do.double())
        # dcoef[h][i] sums B T row terms <dO, O_i> of random sign.  rel_err divides by the tensor's
        # largest entry; with one entry (H = N = 1: the head-size-256 single-branch cases) a draw whose
        # terms cancel leaves nothing to measure against -- one of the first draws had |sum| = 4.1
        # against sum|term| = 673, so a rounding of 2^-9 per term, the bf16 input format's, is already
        # past the bar.  The single entry's terms are <dO, O> / c_0 of the oracle itself: draw again
        # until |sum| >= sqrt(sum term^2) / 2 (about 0.6 of all draws), which keeps the format's
        # floor u sqrt(sum term^2) / |sum| at 2 u.  Decided on the oracle alone.
        if H * N > 1:
            break
        terms = (do.double() * ref.detach()).sum(-1)
        if terms.sum().abs() >= 0.5 * terms.pow(2).sum().sqrt():
            break
    else:
        raise AssertionError("no well-conditioned draw in 32")
    return types.SimpleNamespace(qkv=qkv, coef=coef, do=do, freqs_c=freqs_c, masks=masks if p else None,
                                 out=ref.detach(), gx=x64.grad, gc=c64.grad, dims=(B, T, H, N, hs, dv))


def _gpu(pb, p=0.0, seed=SEED):
    B, T, H, N, hs, dv = pb.dims
    xg = pb.qkv.to(DEV).requires_grad_(True)
    cg = pb.coef.to(DEV).requires_grad_(True)
    freqs = torch.view_as_real(pb.freqs_c[:T]).contiguous().to(DEV) if pb.freqs_c is not None else None
    out = ops.diff_attention(xg, cg, H, N, hs, freqs, dv=dv, dropout_p=p, seed=seed)
    out.backward(pb.do.to(DEV))
    torch.cuda.synchronize()
    assert cg.grad.dtype == torch.float32 and cg.grad.shape == (H, N)
    return out.detach().float().cpu(), xg.grad.float().cpu(), cg.grad.cpu()


def _errors(pb, got):
    B, T, H, N, hs, dv = pb.dims
    out, gx, gc = got
    nq = H * N * hs
    errs = {"O": rel_err(out, pb.out), "dcoef": rel_err(gc, pb.gc)}
    for name, sl in (("dQ", slice(0, nq)), ("dK", slice(nq, 2 * nq)), ("dV", slice(2 * nq, None))):
        errs[name] = rel_err(gx[..., sl], pb.gx[..., sl])
    return errs


def _assert_parity(pb, got, tol, tag=""):
    errs = _errors(pb, got)
    print(tag, {k: f"{v:.3g}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, (tag, bad, tol)


def _run(dtype, H, N, hs, T=T0, rope=False, dv=None, p=0.0, seed=SEED, tag=""):
    dv = 2 * hs if dv is None else dv
    assert ops.attention_supported(dtype, hs, N, dv)           # a missing plan is an error, not a skip
    p = _f32(p)
    pb = _problem(dtype, H, N, hs, T, rope, dv, p, seed)
    got = _gpu(pb, p, seed)
    _assert_parity(pb, got, TOL[dtype], tag)
    return pb, got


@contextlib.contextmanager
def _switch(flag, value):
    """One of ops' one-element test switches (_LSE_C_WORKSPACE, _DV_F32_WORKSPACE) set for a block."""
    old = flag[0]
    flag[0] = value
    try:
        yield
    finally:
        flag[0] = old


# ============================================================ A. the plan matrix ===
HEAD_SIZES = (16, 32, 64, 96, 128, 256)


def _matrix():
    out = []
    for dtype in (F32, BF16, F16):
        for hs in HEAD_SIZES:
            for N, dv in ((1, hs), (1, 2 * hs), (2, 2 * hs), (3, 2 * hs), (4, 2 * hs)):
                for p in (0.0, 0.2):
                    for caps in ((None,) if N == 1 else (None, (4, 4))):
                        ident = f"{NAME[dtype]}-hs{hs}-N{N}-dv{dv}-p{p}-" + ("default" if caps is None else "caps44")
                        out.append(pytest.param(dtype, hs, N, dv, p, caps, id=ident))
    return out


@pytest.mark.parametrize("dtype,hs,N,dv,p,caps", _matrix())
def test_plan_matrix(dtype, hs, N, dv, p, caps):
    """dtype x DTA_FOR_CONFIGS head size x (N, dv) x dropout x backward caps, RoPE on for odd N:
    O, dQ, dK, dV and dcoef against fp64; 16-bit without dropout also with lse_c = NULL.  A shape
    without a plan must raise (fp32 differential plans at head size 256)."""
    H = 1 if hs == 256 else 2
    rope = N % 2 == 1
    with ops.bwd_group_caps(*caps) if caps else contextlib.nullcontext():
        if not ops.attention_supported(dtype, hs, N, dv):
            x = torch.zeros(2, T0, ops.packed_width(H, N, hs, dv), device=DEV, dtype=dtype)
            with pytest.raises(RuntimeError, match="no gfx950 kernel"):
                ops.diff_attention(x, torch.ones(H, N, device=DEV), H, N, hs, None, dv=dv, dropout_p=p, seed=SEED)
            return
        pb, _ = _run(dtype, H, N, hs, rope=rope, dv=dv, p=p, tag="default workspaces")
        if p == 0.0 and dtype != F32:
            with _switch(ops._LSE_C_WORKSPACE, False):
                _assert_parity(pb, _gpu(pb), TOL[dtype], "lse_c off")


# ======================================= B. the remaining dropout combinations ===
SIXTEEN = [BF16, F16]


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("N", [3, 4])
def test_dropout_dv_groups_without_f32_workspace(dtype, N):
    """Grouped dK/dV with dv_f32 = NULL: the later groups read-add-store the 16-bit dV, and
    their mask keys keep the call's branch index (br0 + i, cst)."""
    hs = 64
    assert _lib.load().dta_attn_bwd_dkdv_groups(_lib.dtype_code(dtype), hs, N, 2 * hs, 0) > 1
    with _switch(ops._DV_F32_WORKSPACE, False):
        _run(dtype, 2, N, hs, rope=N % 2 == 1, p=0.2)


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("N,hs", [(2, 64), (4, 32)])
def test_dropout_fp16_branch_outputs(dtype, N, hs, monkeypatch):
    monkeypatch.setenv("DTA_OBR_F16", "1")
    assert ops._obr_dtype(dtype) == F16
    _run(dtype, 2, N, hs, p=0.2)


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("N,hs,dv,hp", [(2, 48, 96, 64), (2, 160, 320, 256), (2, 200, 400, 256),
                                        (1, 40, 40, 64), (1, 200, 200, 256)])
def test_dropout_padded_head_sizes(dtype, N, hs, dv, hp):
    """Head sizes without a plan of their own, zero-padded into the next built one (the
    differential plans and the control's dv = hs), with dropout."""
    assert ops.padded_head(dtype, hs, N, dv) == hp
    _run(dtype, 1 if hp == 256 else 2, N, hs, rope=N == 1, dv=dv, p=0.2)


def _dropped_rows(pb):
    """(b, t, h, i) -> whether every causal key of that map row is dropped."""
    T = pb.dims[1]
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool))
    return ((pb.masks > 0) & causal).sum(-1).eq(0).permute(0, 3, 1, 2)        # (B, T, H, N)


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("T", [1, 33])
def test_dropout_rows_with_every_key_dropped(dtype, T):
    """p = 0.5 at T = 1 and T = 33: some map rows keep no key.  Such a row of branch i has
    dQ_i exactly zero, and where it is dropped in every branch of a head, O exactly zero -- in
    the oracle and in the kernels.  (Only those rows: a row with one causal key has dQ = 0 in the
    oracle by exact cancellation, which no rounding kernel reproduces bit for bit.)"""
    H, N, hs = 2, 2, 64
    pb, (out, gx, _) = _run(dtype, H, N, hs, T=T, p=0.5, seed=SEED + T)
    gone = _dropped_rows(pb)
    assert gone.any() and gone.all(-1).any(), "the seed must drop a whole row of some branch and of some head"
    nq = H * N * hs
    assert (pb.gx[..., :nq].unflatten(-1, (H, N, hs))[gone] == 0).all() and (pb.out.view(2, T, H, -1)[gone.all(-1)] == 0).all()
    assert (out.view(2, T, H, -1)[gone.all(-1)] == 0).all(), "O of a row whose every key is dropped in every branch"
    assert (gx[..., :nq].unflatten(-1, (H, N, hs))[gone] == 0).all(), "dQ_i of a row whose every key is dropped"


CLAMPS = [  # p, T, seed: the threshold clamps of drop_params and the wrap of idx + seed_hi
    pytest.param(1e-10, T0, SEED, id="p1e-10-thr1-scale1"),
    pytest.param(0.9, 200, SEED, id="p0.9-T200"),
    pytest.param(0.2, T0, 0x0000_0001_0000_0000 | 0x9ABC, id="seed-hi-1"),
    pytest.param(0.2, T0, 0xFFFF_FFFF_0000_0000 | 0x9ABC, id="seed-hi-ffffffff-wraps"),
]


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("p,T,seed", CLAMPS)
def test_dropout_threshold_and_seed_clamps(dtype, p, T, seed):
    if p == 1e-10:
        # thr = max(1, p 2^32) = 1 and scale = float(1 / (1 - p)) = 1: at most the hash value 0 drops
        assert int(_f32(p) * 2 ** 32) == 0 and np.float32(1.0 / (1.0 - _f32(p))) == 1.0
    _run(dtype, 2, 2, 64, T=T, p=p, seed=seed)


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
def test_dropout_five_branches(dtype):
    """N = 5: the branch-split forward with a grouped backward; every group's mask key takes the
    call's branch index and count."""
    _run(dtype, 2, 5, 64, rope=True, p=0.2)


# ================================== C. coefficient scale, checked per branch ===
COEF_SCALES = [1e-3, 1e-2, 30.0, 1000.0]
_COEF_ERRS = {}


@pytest.fixture(scope="module", autouse=True)
def _coef_scale_report():
    """With DTA_COEF_SCALE_JSON set, the per-branch errors of section C are written there
    (profiles/coef_scale_errors.json is such a run)."""
    yield
    path = os.environ.get("DTA_COEF_SCALE_JSON")
    if path and _COEF_ERRS:
        with open(path, "w") as fh:
            json.dump({"shape": "B 2, H 2, N 3, hs 64, T 150; coef [1, s, -s], [1, -s, s]",
                       "norms": "dQ / dK: max|err| / max|oracle| of each branch; dcoef: each entry over the "
                                "head's largest oracle entry; O, dV: max-norm of the tensor",
                       "errors": _COEF_ERRS}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _per_branch(pb, got):
    B, T, H, N, hs, dv = pb.dims
    out, gx, gc = got
    nq = H * N * hs
    errs = {"O": rel_err(out, pb.out), "dV": rel_err(gx[..., 2 * nq:], pb.gx[..., 2 * nq:])}
    for name, lo in (("dQ", 0), ("dK", nq)):
        a, r = gx[..., lo:lo + nq].unflatten(-1, (H, N, hs)), pb.gx[..., lo:lo + nq].unflatten(-1, (H, N, hs))
        errs[name] = [rel_err(a[..., i, :], r[..., i, :]) for i in range(N)]
    top = pb.gc.abs().amax(1, keepdim=True)
    errs["dcoef"] = ((gc.double() - pb.gc).abs() / top).tolist()
    return errs


@pytest.mark.parametrize("dtype", SIXTEEN, ids=NAME.get)
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("s", COEF_SCALES)
def test_coefficient_scale_per_branch(dtype, rope, s):
    """coef = [1, +-s, -+s]: dQ_i and dK_i of every branch against that branch's own oracle
    maximum, each dcoef entry against its head's largest, O and dV as usual, with the |c_i|
    fold (the default, lse_c given) and without it.  The gradients are linear in c_i, so a
    kernel that rounds like the algorithm has a per-branch error that does not depend on s;
    the unfolded run is the witness of that in this repository.  Bar: TOL[dtype] per branch."""
    H, N, hs, T = 2, 3, 64, 150
    pb = _problem(dtype, H, N, hs, T, rope, 2 * hs, 0.0, SEED, coef_rows=((1.0, s, -s), (1.0, -s, s)))
    tol, bad = TOL[dtype], {}
    for fold in (True, False):
        with _switch(ops._LSE_C_WORKSPACE, fold):
            errs = _per_branch(pb, _gpu(pb))
        path = "fold" if fold else "unfolded"
        _COEF_ERRS[f"{NAME[dtype]}/{'rope' if rope else 'plain'}/s={s:g}/{path}"] = errs
        print(path, errs)
        flat = {"O": errs["O"], "dV": errs["dV"], "dcoef": max(max(r) for r in errs["dcoef"])}
        flat.update({f"{k}_{i}": e for k in ("dQ", "dK") for i, e in enumerate(errs[k])})
        bad.update({f"{path}:{k}": v for k, v in flat.items() if not v < tol})
    assert not bad, (bad, tol)


# ============================================ D. zero-sized calls, poisoned ===
ATTN_LISTS = ({"o", "obr", "lse", "qk_rot", "dqkv", "dcoef", "delta"}, {"dcp", "dv32", "lsec"})


@pytest.mark.parametrize("dtype", [F32, BF16], ids=NAME.get)
@pytest.mark.parametrize("B,T", [(2, 0), (0, T0)], ids=["T0", "B0"])
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_empty_attention(dtype, B, T, rope, p):
    """No rows: an empty O of the right shape, an empty d(qkv), and d(coef) -- a sum over no
    rows -- exactly zero, on poisoned memory (dcoef comes from torch.empty)."""
    H, N, hs = 2, 2, 64
    dv = 2 * hs
    with poisoned_allocations() as s:
        xg = torch.zeros(B, T, ops.packed_width(H, N, hs, dv), device=DEV, dtype=dtype).requires_grad_(True)
        cg = torch.tensor([[1.0, -0.4], [1.0, 0.3]], device=DEV).requires_grad_(True)
        freqs = torch.view_as_real(orc.precompute_freqs_cis(hs, 8)[:T]).contiguous().to(DEV) if rope else None
        out = ops.diff_attention(xg, cg, H, N, hs, freqs, dropout_p=p, seed=SEED)
        assert out.shape == (B, T, H * dv) and out.dtype == dtype
        out.backward(torch.zeros(B, T, H * dv, device=DEV, dtype=dtype))
        s.verify(*ATTN_LISTS)
    assert "dcoef" in s.names()
    assert xg.grad.shape == xg.shape and xg.grad.dtype == dtype
    assert cg.grad.shape == (H, N) and cg.grad.dtype == torch.float32
    assert (cg.grad.view(torch.int32) == 0).all(), cg.grad


def _poison_f32(n):
    return torch.full((n,), float("nan"), device=DEV)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=NAME.get)
@pytest.mark.parametrize("B,T", [(2, 0), (0, T0)], ids=["T0", "B0"])
def test_empty_attention_backward_c_abi(dtype, B, T):
    """dta_attn_bwd with no rows, every pointer but dcoef / dcoef_partial NULL (nothing else may
    be touched): dcoef is zero after every call whose stages write it -- DQ, with the partials or
    without, and PRE without them -- and a DKDV-only call leaves it alone."""
    lib = _lib.load()
    H, N, hs = 2, 3, 64
    stream = _lib.stream_handle(torch.device(DEV))
    part = _poison_f32(64)

    def call(stages, partial, dcoef):
        a = _lib.AttnBwdArgs()
        a.dtype, a.B, a.T, a.H, a.n_terms, a.head_size, a.dv = _lib.dtype_code(dtype), B, T, H, N, hs, 2 * hs
        a.scale, a.stages, a.dcoef = hs ** -0.5, stages, dcoef.data_ptr()
        a.dcoef_partial = part.data_ptr() if partial else None
        _lib.check(lib.dta_attn_bwd(a, stream))
        torch.cuda.synchronize()

    for partial in (True, False):
        for seq in ((_lib.BWD_DQ, _lib.BWD_DKDV), (0,)):                  # as ops passes them; all at once
            dcoef = _poison_f32(H * N)
            for stages in seq:
                call(stages, partial, dcoef)
            assert (dcoef.view(torch.int32) == 0).all(), (partial, seq, dcoef)
        dcoef = _poison_f32(H * N)
        call(_lib.BWD_DKDV, partial, dcoef)
        assert dcoef.isnan().all(), "a DKDV-only call must not touch dcoef"
        call(_lib.BWD_PRE, partial, dcoef)
        # PRE is the zeroing stage of the atomics path; with the partials it is a no-op
        assert dcoef.isnan().all() if partial else (dcoef.view(torch.int32) == 0).all()
    assert part.isnan().all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=NAME.get)
@pytest.mark.parametrize("shape", [(0, 256), (2, 0, 256)], ids=["rows0", "T0"])
def test_empty_group_ln_scale(dtype, shape):
    C = shape[-1]
    with poisoned_allocations() as s:
        xg = torch.zeros(shape, device=DEV, dtype=dtype).requires_grad_(True)
        wg = torch.ones(C, device=DEV).requires_grad_(True)
        bg = torch.zeros(C, device=DEV).requires_grad_(True)
        out = ops.group_ln_scale(xg, wg, bg, 1e-5, 0.2)
        assert out.shape == shape and out.dtype == dtype
        out.backward(torch.zeros(shape, device=DEV, dtype=dtype))
        s.verify({"y", "mean", "rstd", "dx"}, {"part"})
    assert xg.grad.shape == shape
    for g in (wg.grad, bg.grad):
        assert g.shape == (C,) and (g.view(torch.int32) == 0).all()


def test_empty_add_layer_norm():
    C = 256
    ln = ops.LayerNorm(C, autocast_out=True).to(DEV)
    with poisoned_allocations() as s:
        x = torch.zeros(0, C, device=DEV).requires_grad_(True)
        a = torch.zeros(0, C, device=DEV, dtype=BF16).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            xo, y = ops.add_layer_norm(x, a, ln)
        assert type(y.grad_fn).__name__ == "_AddLNBackward"
        assert xo.shape == (0, C) and xo.dtype == F32 and y.shape == (0, C) and y.dtype == BF16
        torch.autograd.backward([xo, y], [torch.zeros_like(xo), torch.zeros_like(y)])
        s.verify({"y", "mean", "rstd", "dx", "xo", "da"}, {"part"})
    assert x.grad.shape == (0, C) and a.grad.shape == (0, C) and a.grad.dtype == BF16
    for g in (ln.weight.grad, ln.bias.grad):
        assert g.shape == (C,) and (g.view(torch.int32) == 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=NAME.get)
def test_empty_swiglu(dtype):
    n = 64
    with poisoned_allocations() as s:
        ag = torch.zeros(0, n, device=DEV, dtype=dtype).requires_grad_(True)
        bg = torch.zeros(0, n, device=DEV, dtype=dtype).requires_grad_(True)
        out = ops.swiglu(ag, bg)
        assert type(out.grad_fn).__name__ == "_SwiGLUBackward" and out.shape == (0, n) and out.dtype == dtype
        out.backward(torch.zeros(0, n, device=DEV, dtype=dtype))
        assert ag.grad.shape == (0, n) and bg.grad.shape == (0, n)
        # the packed launch as _PackedSwiGLU drives it, with the bias-gradient pass
        y2 = torch.zeros(0, 2 * n, device=DEV, dtype=dtype)
        out2 = torch.empty(0, n, device=DEV, dtype=dtype)
        ops._swiglu_launch(y2, n, out2, None, None)
        dy = torch.empty_like(y2)
        dbias = torch.empty(2 * n, device=DEV, dtype=F32)
        ops._swiglu_launch(y2, n, None, torch.zeros(0, n, device=DEV, dtype=dtype), dy, dbias)
        s.verify({"out", "da", "db", "out2", "dy", "dbias"}, {"work"})
    assert (dbias.view(torch.int32) == 0).all()


def test_empty_rope_rows_accumulate_and_kv_quant_rows():
    H, N, hs, dv, P = 2, 2, 32, 64, 32
    nq = H * N * hs
    with poisoned_allocations() as s:
        src = torch.zeros(2, 0, H, N, hs, device=DEV, dtype=BF16)
        ops.rope_rows(src, torch.zeros_like(src), torch.zeros(0, hs // 2, 2, device=DEV))
        g, d = torch.zeros(0, device=DEV), torch.zeros(0, device=DEV, dtype=BF16)
        packing.accumulate(g, d)
        pool = s.guarded(torch.full((3, P, nq + H * dv), 0xA5, dtype=torch.uint8, device=DEV), "byte_pool")
        scales = s.guarded(torch.full((3, P, H, N + 1), -7.0, device=DEV), "scale_pool")
        ops.kv_quant_rows(torch.zeros(2, 0, H, N, hs, device=DEV, dtype=BF16), torch.zeros(2, 0, H, dv, device=DEV, dtype=BF16),
                          pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv)), scales,
                          torch.zeros(0, device=DEV, dtype=torch.int32))
        s.verify(set(), set())
    assert (pool == 0xA5).all() and (scales == -7.0).all()
