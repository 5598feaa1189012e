"""Every kernel's outputs and scratch on poisoned, guarded memory (tests/_poison.py).

``ops.py`` takes every result and workspace from ``torch.empty``; in a test process that memory
is usually zero or the previous call's correct result, so an element a kernel never writes, a
read of scratch nobody wrote and a store a few elements past a tensor all pass the max-norm bar
of the parity tests.  Here each entry point runs once on plain memory and once inside
``poisoned_allocations()`` -- every ``torch.empty`` / ``torch.empty_like`` a fresh buffer of
0xFF bytes (NaN in every float type) between two 4 KiB guard bands, and the caller's tensors
(inputs, dO, caches, pools, tables) copied into such buffers with ``guarded`` -- and asserts, in
this order:

(a) every guard band of every allocation and every guarded tensor is untouched;
(b) every allocation is named in the entry point's *results* or *scratch* list below (a new
    buffer fails until somebody classifies it by what its consumer reads), and every result
    allocation is finite in every element; scratch may keep unwritten padding;
(c) the returned tensors and gradients are bitwise those of the plain run (the kernels are
    deterministic run to run, so a difference is a dependence on memory they did not write);
(d) parity with the fp64 reference at the bars the parity tests already use (TOL of
    test_gpu_parity.py / test_gpu_ragged.py, the SwiGLU and fused add+LayerNorm bars of
    test_gpu_block_ops.py, test_gpu_fp8_cache.py's reference on the dequantised rows).

The shapes are the smallest that still reach every plan family and every edge: B = 2, T below
one tile, one tile plus one, odd sizes; 1 / 9 / 513 rows; lengths around the decode chunk.

Not reached this way (and not worked round): allocations made inside torch's C++ (rocBLAS
workspaces, autograd's own buffers, ``F.pad`` / ``torch.cat`` of the padded head sizes), the
``torch.zeros`` dw / db of the LayerNorm backward, and ``kv_cache.py``'s cache buffers and RoPE
temporaries (``buf``, ``sc``, ``q_rot``, ``k_rot``), whose model-level steps are not driven here.
"""

import pytest
import torch
from torch.nn import functional as F

import test_gpu_fp8_cache as F8
import test_gpu_paged as PG
import test_gpu_ragged as R
from _poison import poisoned_allocations
from conftest import Golden, rel_err
from oracle import diffattn_oracle as orc
from test_boundary_cpu import _cases
from test_gpu_dropout import _oracle_dropped, drop_masks
from test_gpu_modules import _run_module
from test_gpu_parity import DEV, TOL, _oracle_core, _rope64

from differential_transformer_replication_amd import _lib, ops, packing

pytestmark = pytest.mark.gpu

# ---- classification: what the consumer reads -------------------------------------------
# results: read whole by a consumer (the caller, the backward, autograd); scratch: private
# workspaces whose padding nobody reads
ATTN = ({"o", "obr", "lse", "qk_rot", "dqkv", "dcoef", "delta"}, {"dcp", "dv32", "lsec"})
LN = ({"y", "mean", "rstd", "dx", "xo", "da"}, {"part"})
SWIGLU = ({"out", "da", "db", "dy"}, {"work"})
DECODE = ({"o"}, {"ws"})
EXTEND = ({"o"}, set())
NONE = (set(), set())
EVERY = tuple(set().union(*(c[i] for c in (ATTN, LN, SWIGLU, DECODE, EXTEND))) for i in (0, 1))

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
NAN = float("nan")


def _same(got, plain, what):
    for name, a, b in zip(what, got, plain):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a, b), f"{name}: the poisoned run differs from the plain run (reads memory nobody wrote)"


# ============================================================== attention ===
def _attn_inputs(dtype, H, N, hs, T, rope, dv):
    g = torch.Generator().manual_seed(1000 * H + 100 * N + hs + T + dv)
    B = 2
    qkv = torch.randn(B, T, ops.packed_width(H, N, hs, dv), generator=g).to(dtype)
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    do = torch.randn(B, T, H * dv, generator=g).to(dtype)
    freqs_c = orc.precompute_freqs_cis(hs, max(T, 8)) if rope else None
    return qkv, coef, do, freqs_c


def _attn_run(inp, H, N, hs, dv, p, seed, wrap):
    qkv, coef, do, freqs_c = inp
    T = qkv.shape[1]
    xg = wrap(qkv.to(DEV), "qkv").requires_grad_(True)
    cg = wrap(coef.to(DEV), "coef").requires_grad_(True)
    freqs = wrap(torch.view_as_real(freqs_c[:T]).contiguous().to(DEV), "freqs") if freqs_c is not None else None
    out = ops.diff_attention(xg, cg, H, N, hs, freqs, dv=dv, dropout_p=p, seed=seed)
    out.backward(wrap(do.to(DEV), "do"))
    return out.detach(), xg.grad, cg.grad


def _attn_case(dtype, H, N, hs, T, rope, dv=None, p=0.0):
    dv = 2 * hs if dv is None else dv
    assert ops.attention_supported(dtype, hs, N, dv)            # a missing plan is an error, not a skip
    B, seed = 2, 0x1234_5678_9ABC + T
    inp = _attn_inputs(dtype, H, N, hs, T, rope, dv)
    qkv, coef, do, freqs_c = inp
    plain = _attn_run(inp, H, N, hs, dv, p, seed, lambda t, name: t)
    with poisoned_allocations() as s:
        got = _attn_run(inp, H, N, hs, dv, p, seed, s.guarded)
        s.verify(*ATTN)                                            # (a), (b)
    names = s.names()
    assert {"o", "obr", "lse", "dqkv", "dcoef", "delta", "dcp"} <= set(names), names
    assert ("qk_rot" in names) == rope
    _same(got, plain, ("O", "dqkv", "dcoef"))                      # (c)
    # (d) the fp64 oracle on the inputs as the kernels see them
    x64 = qkv.double().requires_grad_(True)
    c64 = coef.double().clone().requires_grad_(True)
    if p == 0.0 and dv == 2 * hs:
        ref = _oracle_core(x64, c64, H, N, hs, freqs_c)
    else:
        masks = drop_masks(seed, p, B, H, N, T) if p else torch.ones(B, H, N, 1, 1, dtype=torch.float64)
        ref = _oracle_dropped(x64, c64, H, N, hs, dv, masks, freqs_c)
    ref.backward(do.double())
    tol, nq = TOL[dtype], H * N * hs
    out, gx, gc = (t.float().cpu() for t in got)
    assert rel_err(out, ref) < tol, "O"
    for name, sl in (("dQ", slice(0, nq)), ("dK", slice(nq, 2 * nq)), ("dV", slice(2 * nq, None))):
        assert rel_err(gx[..., sl], x64.grad[..., sl]) < tol, name
    assert rel_err(gc, c64.grad) < tol, "dcoef"
    return names


# H, N, hs, T, rope: every built head size, N = 1..4, T below a tile / a tile plus one / odd
ATTN_CASES = [
    (1, 2, 16, 7, False), (3, 2, 32, 200, True), (1, 4, 32, 129, True), (2, 2, 64, 129, False),
    (2, 3, 64, 65, True), (1, 4, 64, 200, False), (2, 1, 64, 65, True), (2, 2, 64, 1, False),
    (2, 2, 96, 129, True), (1, 4, 96, 65, False), (1, 3, 96, 7, True), (2, 2, 128, 200, False),
    (1, 3, 128, 129, True), (1, 1, 128, 65, False),
    (2, 2, 40, 129, True), (1, 3, 40, 7, False),                   # zero-padded into the 64 plan
]
# the head-size-256 plans (16-bit differential models), directly and zero-padded from 160 / 200
ATTN_CASES_256 = [(1, 2, 256, 65, False), (2, 1, 256, 129, True), (1, 3, 256, 7, True), (2, 2, 160, 129, True),
                  (1, 2, 200, 65, False)]
# the control model: N = 1, dv = hs (256 in every dtype)
CONTROL_CASES = [(2, 1, 64, 129, True), (1, 1, 128, 200, False), (1, 1, 256, 65, True), (3, 1, 32, 7, False),
                 (2, 1, 40, 65, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,N,hs,T,rope", ATTN_CASES)
def test_attention(dtype, H, N, hs, T, rope):
    _attn_case(dtype, H, N, hs, T, rope)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,N,hs,T,rope", ATTN_CASES_256)
def test_attention_head_size_256(dtype, H, N, hs, T, rope):
    assert ops.padded_head(dtype, hs, N, 2 * hs) == 256
    _attn_case(dtype, H, N, hs, T, rope)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,N,hs,T,rope", CONTROL_CASES)
def test_attention_control_dv_equals_hs(dtype, H, N, hs, T, rope):
    _attn_case(dtype, H, N, hs, T, rope, dv=hs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,N,hs,T,rope", [(1, 3, 128, 129, False), (1, 4, 64, 65, True), (2, 3, 32, 200, False)])
def test_attention_native_backward_plans(dtype, H, N, hs, T, rope):
    with ops.bwd_group_caps(4, 4):
        _attn_case(dtype, H, N, hs, T, rope)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,N,hs,T,rope", [(2, 3, 64, 129, False), (1, 4, 64, 200, True)])
def test_attention_dv_groups_without_f32_workspace(dtype, H, N, hs, T, rope):
    assert _lib.load().dta_attn_bwd_dkdv_groups(_lib.dtype_code(dtype), hs, N, 2 * hs, 0) > 1
    assert "dv32" in _attn_case(dtype, H, N, hs, T, rope)          # the product's path allocates it
    ops._DV_F32_WORKSPACE[0] = False
    try:
        assert "dv32" not in _attn_case(dtype, H, N, hs, T, rope)
    finally:
        ops._DV_F32_WORKSPACE[0] = True


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,N,hs,T,rope", [(2, 2, 64, 129, False), (2, 3, 64, 65, True)])
def test_attention_without_lse_c(dtype, H, N, hs, T, rope):
    ops._LSE_C_WORKSPACE[0] = False
    try:
        assert "lsec" not in _attn_case(dtype, H, N, hs, T, rope)
    finally:
        ops._LSE_C_WORKSPACE[0] = True


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,N,hs,T,rope", [(2, 2, 64, 129, False), (1, 4, 32, 65, True)])
def test_attention_fp16_branch_outputs(dtype, H, N, hs, T, rope, monkeypatch):
    monkeypatch.setenv("DTA_OBR_F16", "1")
    assert ops._obr_dtype(dtype) == F16
    _attn_case(dtype, H, N, hs, T, rope)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("H,N,hs,T,rope", [(2, 2, 64, 129, False), (1, 3, 32, 200, True)])
def test_attention_dropout(dtype, H, N, hs, T, rope):
    assert "lsec" not in _attn_case(dtype, H, N, hs, T, rope, p=0.1)


# ======================================== GroupLayerNorm / LayerNorm / add + LN ===
LN_ROWS = [1, 9, 513]


@pytest.mark.parametrize("C", [48, 384, 2048, 4104, 8192])
@pytest.mark.parametrize("dtype", [F32, BF16, "mixed"])
def test_layer_norm(dtype, C):
    """_GroupLNScale (GroupLayerNorm and the Blocks' LayerNorm): fp32, bf16, and fp32 x
    normalised into bf16 y with a bf16 dy; reference and bars of test_ln_bwd_row_ring_ragged."""
    xdt, ydt = (F32, BF16) if dtype == "mixed" else (dtype, dtype)
    for rows in LN_ROWS:
        g = torch.Generator().manual_seed(rows * 7 + C)
        x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(xdt)
        w = 1 + 0.1 * torch.randn(C, generator=g)
        b = 0.1 * torch.randn(C, generator=g)
        dy = torch.randn(rows, C, generator=g).to(ydt)

        def run(wrap):
            xg = wrap(x.to(DEV), "x").requires_grad_(True)
            wg, bg = wrap(w.to(DEV), "w").requires_grad_(True), wrap(b.to(DEV), "b").requires_grad_(True)
            out = ops._GroupLNScale.apply(xg, wg, bg, 1e-5, 0.2, None, ydt if dtype == "mixed" else None)
            assert out.dtype == ydt
            out.backward(wrap(dy.to(DEV), "dy"))
            return out.detach(), xg.grad, wg.grad, bg.grad

        plain = run(lambda t, name: t)
        with poisoned_allocations() as s:
            got = run(s.guarded)
            s.verify(*LN)
        assert s.names() == ["y", "mean", "rstd", "dx", "part"]
        _same(got, plain, ("y", "dx", "dw", "db"))
        xq = x.double().requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        ref = orc.group_layer_norm(xq, w64, b64) * 0.2
        ref.backward(dy.double())
        tol = TOL[BF16] if ydt == BF16 else TOL[F32]
        for name, a, r in zip(("y", "dx", "dw", "db"), got, (ref, xq.grad, w64.grad, b64.grad)):
            assert rel_err(a.float().cpu(), r) < tol, (name, rows)


@pytest.mark.parametrize("C", [48, 384, 2048, 4104, 8192])
def test_add_layer_norm_fused(C):
    """ops.add_layer_norm on its fused path (fp32 stream, bf16 branch, bf16 LN
    output under autocast); reference and bars of test_add_layer_norm_fused_equals_unfused,
    x + a itself at the fp32 bar."""
    torch.manual_seed(C)
    ln = ops.LayerNorm(C, autocast_out=True).to(DEV)
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.1)
        ln.bias.normal_(0.0, 0.1)
    for rows in LN_ROWS:
        g = torch.Generator().manual_seed(rows + C)
        x0, gx = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
        a0, gy = torch.randn(rows, C, generator=g).to(BF16), torch.randn(rows, C, generator=g).to(BF16)

        def run(wrap):
            x = wrap(x0.to(DEV), "x").requires_grad_(True)
            a = wrap(a0.to(DEV), "a").requires_grad_(True)
            ln.weight.grad = ln.bias.grad = None
            with torch.autocast("cuda", dtype=BF16):
                xo, y = ops.add_layer_norm(x, a, ln)
            assert type(y.grad_fn).__name__ == "_AddLNBackward" and xo.dtype == F32 and y.dtype == BF16
            torch.autograd.backward([xo, y], [wrap(gx.to(DEV), "gx"), wrap(gy.to(DEV), "gy")])
            return xo.detach(), y.detach(), x.grad, a.grad, ln.weight.grad, ln.bias.grad

        plain = run(lambda t, name: t)
        with poisoned_allocations() as s:
            got = run(s.guarded)
            s.verify(*LN)
        assert s.names() == ["xo", "y", "mean", "rstd", "dx", "da", "part"]
        _same(got, plain, ("xo", "y", "dx", "da", "dw", "db"))
        x64, a64 = x0.double().requires_grad_(True), a0.double().requires_grad_(True)
        w64 = ln.weight.detach().double().cpu().requires_grad_(True)
        b64 = ln.bias.detach().double().cpu().requires_grad_(True)
        s64 = x64 + a64
        y64 = F.layer_norm(s64, (C,), w64, b64, ln.eps)
        ((s64 * gx.double()).sum() + (y64 * gy.double()).sum()).backward()
        assert rel_err(got[0].cpu(), s64.detach()) < TOL[F32], ("xo", rows)
        for name, a, r in zip(("y", "dx", "da", "dw", "db"), got[1:], (y64.detach(), x64.grad, a64.grad, w64.grad, b64.grad)):
            assert rel_err(a.float().cpu(), r) < 2e-2, (name, rows)


# ================================================================= SwiGLU ===
SWIGLU_SHAPES = [(1, 64), (300, 256), (129, 1536)]


def _swiglu_tol(dtype):
    return 1e-5 if dtype == F32 else 1e-2                           # test_swiglu_matches_torch


def _swiglu_ref(a, b, d):
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    r = F.silu(a64) * b64
    r.backward(d.double())
    return r.detach(), a64.grad, b64.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,n", SWIGLU_SHAPES)
def test_swiglu(dtype, rows, n):
    g = torch.Generator().manual_seed(rows + n)
    a = (torch.randn(rows, n, generator=g) * 3).to(dtype)
    b, d = torch.randn(rows, n, generator=g).to(dtype), torch.randn(rows, n, generator=g).to(dtype)

    def run(wrap):
        ag, bg = wrap(a.to(DEV), "a").requires_grad_(True), wrap(b.to(DEV), "b").requires_grad_(True)
        out = ops.swiglu(ag, bg)
        assert type(out.grad_fn).__name__ == "_SwiGLUBackward" and out.dtype == dtype
        out.backward(wrap(d.to(DEV), "d"))
        return out.detach(), ag.grad, bg.grad

    plain = run(lambda t, name: t)
    with poisoned_allocations() as s:
        got = run(s.guarded)
        s.verify(*SWIGLU)
    assert s.names() == ["out", "da", "db"]
    _same(got, plain, ("out", "da", "db"))
    for name, x, r in zip(("out", "da", "db"), got, _swiglu_ref(a, b, d)):
        assert rel_err(x.float().cpu(), r) < _swiglu_tol(dtype), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,n", SWIGLU_SHAPES)
def test_swiglu_packed_launch(dtype, rows, n):
    """_swiglu_launch over the halves of a packed (rows, 2n) projection as _PackedSwiGLU drives
    it: forward, backward, and backward with the bias-gradient pass (``work`` has 4 floats of
    slack the reduce must not read).  dbias is the fp32 column sum of dA | dB as stored (bar 1e-5,
    test_swiglu_bias_gradient_pass); in fp16 this caught sums of singly rounded products next to
    stores of doubly rounded ones (2.6e-5), fixed in swiglu_bwd_bias_kernel."""
    g = torch.Generator().manual_seed(rows * 3 + n)
    y2 = (torch.randn(rows, 2 * n, generator=g) * 2).to(dtype)
    d2 = torch.randn(rows, n, generator=g).to(dtype)

    def run(wrap):
        y, d = wrap(y2.to(DEV), "y2"), wrap(d2.to(DEV), "d2")
        out = torch.empty(rows, n, device=DEV, dtype=dtype)
        ops._swiglu_launch(y, n, out, None, None)
        dy_nobias = torch.empty_like(y)
        ops._swiglu_launch(y, n, None, d, dy_nobias)
        dy = torch.empty_like(y)
        db = torch.empty(2 * n, device=DEV, dtype=F32)
        ops._swiglu_launch(y, n, None, d, dy, db)
        torch.cuda.synchronize()
        return out, dy_nobias, dy, db

    plain = run(lambda t, name: t)
    with poisoned_allocations() as s:
        got = run(s.guarded)
        s.verify(SWIGLU[0] | {"dy_nobias"}, SWIGLU[1])
    assert s.names() == ["out", "dy_nobias", "dy", "db", "work"]
    _same(got, plain, ("out", "dy_nobias", "dy", "db"))
    out, dy_nobias, dy, db = got
    assert torch.equal(dy, dy_nobias)                              # test_swiglu_bias_gradient_pass
    assert rel_err(db.cpu(), dy.double().sum(0).cpu()) < 1e-5
    r, da, dbb = _swiglu_ref(y2[:, :n], y2[:, n:], d2)
    tol = _swiglu_tol(dtype)
    assert rel_err(out.float().cpu(), r) < tol
    assert rel_err(dy[:, :n].float().cpu(), da) < tol and rel_err(dy[:, n:].float().cpu(), dbb) < tol


# ========================================================= rope_rows, accumulate ===
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,N,hs", [(2, 7, 2, 2, 16), (2, 65, 1, 3, 64), (1, 129, 2, 1, 96)])
def test_rope_rows(dtype, B, T, H, N, hs):
    """dst a strided half of a wider caller-made buffer (as qk_rot[:, :, H:] is): every element
    of dst written, the other half and the guards untouched."""
    g = torch.Generator().manual_seed(T + hs)
    src = torch.randn(B, T, H, N, hs, generator=g).to(dtype)
    freqs_c = orc.precompute_freqs_cis(hs, max(T, 8))
    table = torch.view_as_real(freqs_c[:T]).contiguous()

    def run(wrap):
        buf = wrap(torch.full((B, T, 2 * H, N, hs), NAN, dtype=dtype, device=DEV), "buf")
        ops.rope_rows(wrap(src.to(DEV), "src"), buf[:, :, H:], wrap(table.to(DEV), "table"))
        torch.cuda.synchronize()
        return (buf,)

    plain = run(lambda t, name: t)
    with poisoned_allocations() as s:
        got = run(s.guarded)
        s.verify(*NONE)
    buf = got[0]
    assert buf[:, :, :H].isnan().all() and torch.isfinite(buf[:, :, H:]).all()
    assert torch.equal(buf[:, :, H:], plain[0][:, :, H:])
    want = torch.stack([torch.stack([_rope64(src[:, :, h, i].double(), freqs_c) for i in range(N)], 2)
                        for h in range(H)], 2)
    assert rel_err(buf[:, :, H:].float().cpu(), want) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 1000, (1 << 20) + 5])
def test_accumulate(dtype, n):
    """packing.accumulate on guarded operands: the vector body and the tail stay inside both;
    bitwise torch's fp32 add of the upcast gradient (test_accumulate_f32)."""
    gen = torch.Generator().manual_seed(n)
    g0, d0 = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(dtype).to(DEV)
    ref = g0 + d0.float()
    with poisoned_allocations() as s:
        g, d = s.guarded(g0, "g"), s.guarded(d0, "d")
        assert g.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0      # the HIP launch
        packing.accumulate(g, d)
        s.verify(*NONE)
    assert torch.equal(g, ref) and torch.equal(d, d0)


# ================================================================= decode ===
CHUNK = 256                                                         # DTA_DECODE_CHUNK (csrc/dta_internal.h)
# 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 mixed over the batch, under a capacity of three chunks:
# the chunks past a short sequence leave ``ws`` unwritten, and the combine must not read them
DEC_LENGTHS = [(0, 1, CHUNK + 1), (CHUNK - 1, CHUNK, CHUNK + 1), (CHUNK, 0, 1)]
DEC_SHAPES = [(2, 64, 128), (2, 16, 32)]                            # R.DEC_SHAPES: the split plan, the single-pass plan
assert set(DEC_SHAPES) <= set(R.DEC_SHAPES)
B, H = R.B, R.H


def _dec_tensors(dtype, N, hs, dv, lengths):
    q, k, v, coef = R._dec_inputs(N, hs, dv)
    qd, kd, vd = (t.to(DEV, dtype) for t in (q, k, v))
    for b, L in enumerate(lengths):                                 # as R._dec_run(poison=True)
        kd[b, L:] = NAN
        vd[b, L:] = NAN
    return qd, kd, vd, coef.to(DEV)


def _dec_parity(got, want, lengths, dtype, dv, tag):
    assert got.shape == (B, H * dv) and got.dtype == dtype
    got = got.view(B, H, dv).float().cpu()
    assert torch.isfinite(got).all(), tag
    for b, L in enumerate(lengths):
        if L == 0:
            assert (got[b] == 0).all(), (tag, "an empty sequence writes zeros")
        else:
            assert rel_err(got[b], want[b]) <= R.TOL[dtype], (tag, lengths, b)


def _poisoned_call(call, tensors, names, lists):
    """call(*tensors) plain, then on guarded copies inside the harness: (a), (b), (c)."""
    plain = call(*tensors)
    with poisoned_allocations() as s:
        got = call(*(s.guarded(t, n) for t, n in zip(tensors, names)))
        s.verify(*lists)
    assert s.names() == sorted(lists[0] | lists[1], key=["o", "ws"].index), s.names()
    _same((got,), (plain,), ("o",))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", DEC_SHAPES)
def test_decode(dtype, N, hs, dv):
    for L in (1, CHUNK - 1, CHUNK, CHUNK + 1):
        qd, kd, vd, cd = _dec_tensors(dtype, N, hs, dv, (L,) * B)
        got = _poisoned_call(lambda q, k, v, c: ops.diff_attention_decode(q, k, v, c, L), (qd, kd, vd, cd),
                             ("q", "k_cache", "v_cache", "coef"), DECODE)
        _dec_parity(got, R._dec_want(N, hs, dv, (L,) * B), (L,) * B, dtype, dv, "decode")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", DEC_SHAPES)
def test_decode_ragged(dtype, N, hs, dv):
    for lengths in DEC_LENGTHS:
        tensors = _dec_tensors(dtype, N, hs, dv, lengths) + (R._i32(lengths),)
        got = _poisoned_call(ops.diff_attention_decode_ragged, tensors, ("q", "k_cache", "v_cache", "coef", "lengths"),
                             DECODE)
        _dec_parity(got, R._dec_want(N, hs, dv, lengths), lengths, dtype, dv, "decode_ragged")


def _repool(s, view, nq, unflat_k, unflat_v, name):
    """The packed pool behind a ``_paginate`` view, copied into a guarded buffer and cut into
    the same K | V views."""
    pool = s.guarded(view._base, name) if s is not None else view._base
    return pool[..., :nq].unflatten(-1, unflat_k), pool[..., nq:].unflatten(-1, unflat_v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", DEC_SHAPES)
def test_decode_paged(dtype, N, hs, dv):
    P, nq = 32, H * N * hs
    q, k, v, coef = R._dec_inputs(N, hs, dv)
    qd, kd, vd, cd = q.to(DEV, dtype), k.to(DEV, dtype), v.to(DEV, dtype), coef.to(DEV)
    for lengths in DEC_LENGTHS:
        k_pool, v_pool, table, _, _ = PG._paginate(kd, vd, lengths, P, PG._round_up(R.DEC_CAP, P), seed=P + sum(lengths))
        assert k_pool._base.shape[1:] == (P, nq + H * dv)
        ln = R._i32(lengths)
        plain = ops.diff_attention_decode_paged(qd, k_pool, v_pool, cd, table, ln)
        with poisoned_allocations() as s:
            kp, vp = _repool(s, k_pool, nq, (H, N, hs), (H, dv), "pool")
            got = ops.diff_attention_decode_paged(s.guarded(qd, "q"), kp, vp, s.guarded(cd, "coef"),
                                                  s.guarded(table, "block_table"), s.guarded(ln, "lengths"))
            s.verify(*DECODE)
        assert s.names() == ["o", "ws"]
        _same((got,), (plain,), ("o",))
        _dec_parity(got, R._dec_want(N, hs, dv, lengths), lengths, dtype, dv, "decode_paged")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", [(2, 64, 128), (2, 40, 80)])     # F8.SHAPES: a split plan, the single-pass kernel
def test_decode_paged_fp8(dtype, N, hs, dv):
    assert (N, hs, dv) in F8.SHAPES
    P, nq = 32, H * N * hs
    q, coef, kb, vb, sc = F8._inputs(N, hs, dv)
    qd, cd = q.to(DEV, dtype), coef.to(DEV)
    for lengths in DEC_LENGTHS:
        k_pool, v_pool, scales, table = F8._paginate(kb, vb, sc, lengths, P, F8.CAP, seed=P + sum(lengths))
        ln = R._i32(lengths)
        plain = ops.diff_attention_decode_paged_fp8(qd, k_pool, v_pool, scales, cd, table, ln)
        with poisoned_allocations() as s:
            kp, vp = _repool(s, k_pool, nq, (H, N, hs), (H, dv), "byte_pool")
            got = ops.diff_attention_decode_paged_fp8(s.guarded(qd, "q"), kp, vp, s.guarded(scales, "scale_pool"),
                                                      s.guarded(cd, "coef"), s.guarded(table, "block_table"),
                                                      s.guarded(ln, "lengths"))
            s.verify(*DECODE)
        assert s.names() == ["o", "ws"]
        _same((got,), (plain,), ("o",))
        _dec_parity(got, F8._want(N, hs, dv, lengths, dtype), lengths, dtype, dv, "decode_fp8")


# ================================================================= extend ===
# R.EXT_CASES[:2]: pos / counts straddling a 32-row page and a 64-row tile (31 + 1, 63 + 0, 64 + 32,
# 200 + 20, 0 + 33), padding rows, an empty sequence
EXT_CASES = R.EXT_CASES[:2]


def _ext_parity(got, want, n, Tq, dtype, dv, tag):
    assert got.shape == (B, Tq, H * dv) and got.dtype == dtype
    got = got.view(B, Tq, H, dv).float().cpu()
    assert torch.isfinite(got).all(), tag
    for b in range(B):
        assert (got[b, n[b]:] == 0).all(), (tag, b, "padding rows are zeros")
        if n[b]:
            assert rel_err(got[b, :n[b]], want[b, :n[b]]) <= R.TOL[dtype], (tag, b)


def _ext_tensors(dtype, q, k, v, coef, valid):
    qd, kd, vd = (t.to(DEV, dtype) for t in (q, k, v))
    for b, L in enumerate(valid):                                   # as R._ext_run(poison=True)
        kd[b, L:] = NAN
        vd[b, L:] = NAN
    return qd, kd, vd, coef.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", R.EXT_SHAPES)
def test_extend(dtype, N, hs, dv):
    assert ops.extend_supported(dtype, hs, N, dv)
    for pos, Tq, cap in ((31, 40, 128), (0, 65, 65)):                # rows 31..70: a page and a tile boundary inside
        q, k, v, coef, want = R._ext_case(N, hs, dv, (pos,) * B, None, Tq, cap)
        tensors = _ext_tensors(dtype, q, k, v, coef, (pos + Tq,) * B)
        plain = ops.diff_attention_extend(*tensors, pos)
        with poisoned_allocations() as s:
            got = ops.diff_attention_extend(*(s.guarded(t, n) for t, n in zip(tensors, "qkvc")), pos)
            s.verify(*EXTEND)
        assert s.names() == ["o"]
        _same((got,), (plain,), ("o",))
        _ext_parity(got, want, (Tq,) * B, Tq, dtype, dv, ("extend", pos))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", R.EXT_SHAPES)
def test_extend_ragged_and_paged(dtype, N, hs, dv):
    assert ops.extend_supported(dtype, hs, N, dv)
    P, nq = 32, H * N * hs
    for pos, counts, Tq, cap0 in EXT_CASES:
        q, k, v, coef, want = R._ext_case(N, hs, dv, pos, counts, Tq, cap0)
        valid = [p + c for p, c in zip(pos, counts)]
        tensors = _ext_tensors(dtype, q, k, v, coef, valid) + (R._i32(pos), R._i32(counts))
        plain = ops.diff_attention_extend_ragged(*tensors)
        with poisoned_allocations() as s:
            got = ops.diff_attention_extend_ragged(*(s.guarded(t, n) for t, n in
                                                     zip(tensors, ("q", "k", "v", "coef", "pos", "counts"))))
            s.verify(*EXTEND)
        assert s.names() == ["o"]
        _same((got,), (plain,), ("o",))
        _ext_parity(got, want, counts, Tq, dtype, dv, ("extend_ragged", pos))

        qd, kd, vd, cd, pd, cnt = tensors
        k_pool, v_pool, table, _, _ = PG._paginate(kd, vd, valid, P, PG._round_up(cap0, P), seed=P + Tq)
        plain_paged = ops.diff_attention_extend_paged(qd, k_pool, v_pool, cd, table, pd, cnt)
        assert torch.equal(plain_paged, plain)                       # the ordering contract of test_gpu_paged
        with poisoned_allocations() as s:
            kp, vp = _repool(s, k_pool, nq, (H, N, hs), (H, dv), "pool")
            got = ops.diff_attention_extend_paged(s.guarded(qd, "q"), kp, vp, s.guarded(cd, "coef"),
                                                  s.guarded(table, "block_table"), s.guarded(pd, "pos"),
                                                  s.guarded(cnt, "counts"))
            s.verify(*EXTEND)
        assert s.names() == ["o"]
        _same((got,), (plain_paged,), ("o",))
        _ext_parity(got, want, counts, Tq, dtype, dv, ("extend_paged", pos))


# ========================================================== kv_quant_rows ===
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,hs,dv", [(2, 32, 64), (2, 128, 256), (3, 128, 256)])    # 16, 32, 64 lanes per (row, head)
def test_kv_quant_rows(dtype, N, hs, dv):
    """Pre-filled, guarded byte and scale pools: the addressed rows are ops.kv_quant_reference's
    bytes and scales, every other row and scale is bitwise what it was."""
    Bq, Tn, Hq, P, n_pages = 2, 3, 2, 32, 4
    nq = Hq * N * hs
    W = nq + Hq * dv
    g = torch.Generator().manual_seed(17 * N + hs)
    k_new = (torch.randn(Bq, Tn, Hq, N, hs, generator=g) * torch.logspace(-2, 1, Tn)[None, :, None, None, None]).to(DEV, dtype)
    wide = torch.randn(Bq, Tn, 2 * nq + Hq * dv, generator=g).to(DEV, dtype)
    k_new[0, 1, 1, 0] = 0                                           # a zero K_i row
    wide[1, 0, 2 * nq:2 * nq + dv] = 0                              # a zero V row
    last = (n_pages + 1) * P - 1                                    # the spare page's last row
    slots = [3 * P + 5, 0, n_pages * P - 1, 1 * P + 31, last, 2 * P]
    with poisoned_allocations() as s:
        pool = s.guarded(torch.full((n_pages + 1, P, W), 0xA5, dtype=torch.uint8, device=DEV), "byte_pool")
        scales = s.guarded(torch.full((n_pages + 1, P, Hq, N + 1), -7.0, device=DEV), "scale_pool")
        kg, wg = s.guarded(k_new, "k_new"), s.guarded(wide, "wide")
        v_new = wg[..., 2 * nq:].unflatten(-1, (Hq, dv))            # V as a slice of the packed projection
        ops.kv_quant_rows(kg, v_new, pool[..., :nq].unflatten(-1, (Hq, N, hs)), pool[..., nq:].unflatten(-1, (Hq, dv)),
                          scales, s.guarded(R._i32(slots), "slots"))
        s.verify(*NONE)
    assert torch.equal(kg, k_new) and torch.equal(wg, wide)
    keep = torch.ones((n_pages + 1) * P, dtype=torch.bool, device=DEV)
    keep[slots] = False
    assert (pool.view(-1, W)[keep] == 0xA5).all() and (scales.view(-1, Hq, N + 1)[keep] == -7.0).all()
    rows = pool.view(-1, W)[slots]
    kb, ks = ops.kv_quant_reference(k_new.cpu())                    # IEEE division and RNE conversion on the host
    vb, vs = ops.kv_quant_reference(wide[..., 2 * nq:].unflatten(-1, (Hq, dv)).cpu())
    got_s = scales.view(-1, Hq, N + 1)[slots].view(Bq, Tn, Hq, N + 1).cpu()
    assert torch.equal(got_s[..., :N], ks) and torch.equal(got_s[..., N], vs)
    assert torch.equal(rows[:, :nq].reshape(Bq, Tn, Hq, N, hs).cpu(), kb)
    assert torch.equal(rows[:, nq:].reshape(Bq, Tn, Hq, dv).cpu(), vb)
    assert (got_s[0, 1, 1, 0] == 0) and (got_s[1, 0, 0, N] == 0)


# ============================================================ module level ===
@pytest.mark.parametrize("prefix", ["mhdiff", "mhalt"])
def test_module_bf16_autocast_on_poisoned_memory(golden, prefix):
    """The golden cases of test_module_bf16_autocast through _run_module, once plain and once
    poisoned: guards intact, outputs and every gradient finite and bitwise equal.  One run per
    case (not a loop that chases the intermittent failure)."""
    for case in _cases(golden, prefix):
        g = Golden(golden, case)
        m0, x0, out0 = _run_module(case, g, torch.autocast("cuda", dtype=BF16))
        with poisoned_allocations() as s:
            m1, x1, out1 = _run_module(case, g, torch.autocast("cuda", dtype=BF16))
            s.verify(*EVERY)
        assert {"o", "obr", "lse", "dqkv", "dcoef", "delta", "y", "dx"} <= set(s.names()), case
        names = ["out", "grad_in0"] + [k for k, _ in m0.named_parameters()]
        plain = [out0.detach(), x0.grad] + [p.grad for p in m0.parameters()]
        got = [out1.detach(), x1.grad] + [p.grad for p in m1.parameters()]
        assert [t is None for t in got] == [t is None for t in plain], case
        live = [i for i, t in enumerate(got) if t is not None]
        assert len(live) > 4 and all(torch.isfinite(got[i]).all() for i in live), case
        _same([got[i] for i in live], [plain[i] for i in live], [names[i] for i in live])
