"""The row-wise kernels around the attention core (csrc/elementwise.hip) at every width band,
dtype, stride and edge: GroupLayerNorm / LayerNorm forward and backward and the add + LN fusion,
RoPE, SwiGLU and its bias pass, cast_f32 and accumulate.

Every comparison is against fp64 on the CPU from the inputs as stored (tests/_rowwise.py):

- LN.  All five forward instantiations (CH 1, 2, 4, 8, 16) and the three backward ones
  (CHB 1, 2, 4) at both edges of their width bands, in the five type combinations, at 1, 9, 37
  and 513 rows; contiguous through ``ops._GroupLNScale`` / ``ops.add_layer_norm``, strided
  through ``_lib.LnArgs`` with a different row stride per operand and sentinels in the gaps.
  Rows differ in scale and offset and four are planted (constant, zeros, one outlier, zero dy);
  y, dx (xo, da) are judged row by row at ``max(TOL, 2 x the plain fp32 algorithm's error in
  that row)``, dw / db / mean / rstd at fp32's TOL in every combination.
- One nonzero dy row at a time shows a row the backward skips or counts twice at full size.
- dw / db are added into (bitwise: one fp32 add), reproducible with a workspace, and correct by
  atomics without one.
- RoPE directly: forward and inverse, 16-bit and fp32 -> 16-bit, H N not a power of two,
  strided source and destination, and a grid-stride loop that wraps.
- SwiGLU at the tails of the sigmoid, strided; its bias pass at row-block counts that leave the
  second-stage reduce's runs empty or uneven; cast_f32 bitwise against torch; swiglu, cast_f32
  and accumulate each once over their grid cap.

With DTA_ROWWISE_ERRORS_JSON set, every LN case's kernel error, yardstick and bar are written
there (profiles/rowwise_errors.json is such a run).
"""
import functools
import json
import os

import pytest
import torch

import _rowwise as rw
from oracle import diffattn_oracle as orc

from differential_transformer_replication_amd import _lib, ops, packing

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = rw.F32, rw.BF16, rw.F16
TOL = rw.TOL
SENTINEL = -1232.0                 # exact in every storage dtype
GRID_CAP = 16384 * 256             # items of one trip of swiglu / cast_f32 / rope (grid_for)

_REPORT = {}


def _sig(v):
    return float(f"{v:.4g}")


@pytest.fixture(scope="module", autouse=True)
def _rowwise_report():
    yield
    path = os.environ.get("DTA_ROWWISE_ERRORS_JSON")
    if path and _REPORT:
        above = sorted(f"{c}:{n}" for c, ts in _REPORT.items() for n, t in ts.items() if t["bar"] > t["tol"])
        bands = sorted({(t["band"], c.split("/")[1].split("-C")[0]) for c, ts in _REPORT.items() for t in ts.values()})
        with open(path, "w") as fh:
            json.dump({"norm": "y, dx, xo, da: max|kernel - oracle| / max|oracle| of each row, the worst row reported; "
                               "dw, db: the same over the whole vector; mean: |error| x the row's rstd; rstd: relative",
                       "bar": "row by row max(tol, 2 x yardstick): the plain fp32 algorithm with one rounding to the "
                              "storage dtype (tests/_rowwise.py ln_problem), against the same fp64 oracle; dw, db, mean, "
                              "rstd: fp32's 1e-4 outright",
                       "fields": "kernel / where: the kernels' worst row error and that row; bar: that row's bar; "
                                 "yardstick: the plain algorithm's worst row; band: the forward's CH",
                       "bars_above_tol": above,
                       "band_x_combo": [f"CH{b}:{c}" for b, c in bands],
                       "cases": _REPORT}, fh, indent=0, sort_keys=True)
            fh.write("\n")


def _stream():
    return _lib.stream_handle(torch.device(DEV))


# =============================================================================== LN ===
def _check_ln(case, pb, got):
    res = rw.judge_ln(pb, got)
    tols = rw.ln_tols(pb.combo)
    _REPORT[case] = {n: {"kernel": _sig(r.kernel), "where": r.where, "yardstick": _sig(r.yardstick), "bar": _sig(r.bar),
                         "tol": tols.get(n, TOL[F32]), "band": rw.ln_band(pb.C)} for n, r in res.items()}
    print(case, {n: f"{r.kernel:.3g} / {r.bar:.3g} (yardstick {r.yardstick:.3g}) at {r.where}" for n, r in res.items()})
    for name in tols:
        if name in got:
            assert torch.isfinite(got[name]).all(), (case, name)
            zero = rw.row_errors(got[name].float().cpu(), pb.oracle[name])[1]
            assert torch.equal(zero, rw.expected_zero_rows(pb, name)), (case, name, "zero-oracle rows")
            assert res[name].excess <= tols[name], (case, name, "in the zero-oracle rows", res[name].excess)
    bad = {n: r.over[:4] for n, r in res.items() if r.over}
    assert not bad, (case, bad)


def _run_ops(pb):
    """The public path: ops._GroupLNScale, or ops.add_layer_norm under autocast for the fusion."""
    xdt, ydt = rw.COMBOS[pb.combo]
    xg = pb.x.to(DEV).requires_grad_(True)
    if pb.fused:
        ln = ops.LayerNorm(pb.C, eps=pb.eps, autocast_out=True).to(DEV)
        with torch.no_grad():
            ln.weight.copy_(pb.w)
            ln.bias.copy_(pb.b)
        ag = pb.res.to(DEV).requires_grad_(True)
        with torch.autocast("cuda", dtype=ydt):
            xo, y = ops.add_layer_norm(xg, ag, ln)
        assert type(y.grad_fn).__name__ == "_AddLNBackward" and y.dtype == ydt and xo.dtype == F32
        saved = y.grad_fn.saved_tensors
        torch.autograd.backward([xo, y], [pb.dres.to(DEV), pb.dy.to(DEV)])
        assert ag.grad.dtype == ydt
        got = dict(y=y, xo=xo, dx=xg.grad, da=ag.grad, dw=ln.weight.grad, db=ln.bias.grad)
    else:
        wg, bg = pb.w.to(DEV).requires_grad_(True), pb.b.to(DEV).requires_grad_(True)
        y = ops._GroupLNScale.apply(xg, wg, bg, pb.eps, pb.out_scale, None, ydt if ydt != xdt else None)
        assert type(y.grad_fn).__name__ == "_GroupLNScaleBackward" and y.dtype == ydt
        saved = y.grad_fn.saved_tensors
        y.backward(pb.dy.to(DEV))
        got = dict(y=y, dx=xg.grad, dw=wg.grad, db=bg.grad)
    assert got["dx"].dtype == xdt
    got.update(mean=saved[2], rstd=saved[3])
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in got.items()}


def _buf(t, rows, C, stride, dtype):
    """(rows, stride) of SENTINEL with ``t`` (or nothing yet) in the first C columns."""
    buf = torch.full((rows, stride), SENTINEL, dtype=dtype, device=DEV)
    if t is not None:
        buf[:, :C] = t.to(DEV)
    return buf


def _gaps_untouched(bufs, C):
    for name, b in bufs.items():
        assert (b[:, C:] == SENTINEL).all(), f"{name}: the gap between rows was written"


def _ln_args(pb, **kw):
    xdt, ydt = rw.COMBOS[pb.combo]
    io = 0 if xdt == ydt else 1 + _lib.dtype_code(ydt)
    return _lib.LnArgs(dtype=_lib.dtype_code(xdt), rows=pb.rows, C=pb.C, eps=pb.eps, out_scale=pb.out_scale, io_dtype=io, **kw)


def _run_direct(pb, pad=8, partial=True, prefill=None):
    """dta_ln_fwd / dta_ln_bwd on operands that each have a row stride of their own (C + pad,
    C + 2 pad, ...; pad 0: packed); returns the results and the buffers whose gaps to check."""
    lib = _lib.load()
    xdt, ydt = rw.COMBOS[pb.combo]
    rows, C = pb.rows, pb.C
    st = {n: C + (i + 1) * pad for i, n in enumerate(("x", "y", "dy", "dx", "res", "xo", "dres", "dx16"))}
    x = _buf(pb.x, rows, C, st["x"], xdt)
    y = _buf(None, rows, C, st["y"], ydt)
    w, b = pb.w.to(DEV), pb.b.to(DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    bufs = dict(x=x, y=y)
    kw = {}
    if pb.fused:
        res, xo = _buf(pb.res, rows, C, st["res"], ydt), _buf(None, rows, C, st["xo"], F32)
        kw = dict(res=res.data_ptr(), res_stride=st["res"], xo=xo.data_ptr(), xo_stride=st["xo"])
        bufs.update(res=res, xo=xo)
    a = _ln_args(pb, x=x.data_ptr(), x_stride=st["x"], y=y.data_ptr(), y_stride=st["y"], w=w.data_ptr(), b=b.data_ptr(),
                 mean=mean.data_ptr(), rstd=rstd.data_ptr(), **kw)
    _lib.check(lib.dta_ln_fwd(a, _stream()))
    dy, dx = _buf(pb.dy, rows, C, st["dy"], ydt), _buf(None, rows, C, st["dx"], xdt)
    dw = torch.zeros(C, device=DEV) if prefill is None else prefill[0].clone()
    db = torch.zeros(C, device=DEV) if prefill is None else prefill[1].clone()
    part = torch.empty(lib.dta_ln_bwd_workspace_bytes(rows, C) // 4, device=DEV) if partial else None
    bufs.update(dy=dy, dx=dx)
    kw = {}
    src, src_stride = x, st["x"]
    if pb.fused:
        dres, da = _buf(pb.dres, rows, C, st["dres"], F32), _buf(None, rows, C, st["dx16"], ydt)
        kw = dict(dres=dres.data_ptr(), dres_stride=st["dres"], dx16=da.data_ptr(), dx16_stride=st["dx16"])
        bufs.update(dres=dres, da=da)
        src, src_stride = xo, st["xo"]                  # the backward normalises the sum the forward stored
    a = _ln_args(pb, x=src.data_ptr(), x_stride=src_stride, w=w.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                 dy=dy.data_ptr(), dy_stride=st["dy"], dx=dx.data_ptr(), dx_stride=st["dx"], dw=dw.data_ptr(),
                 db=db.data_ptr(), partial=_lib.ptr(part), **kw)
    _lib.check(lib.dta_ln_bwd(a, _stream()))
    torch.cuda.synchronize()
    got = dict(y=y[:, :C], dx=dx[:, :C], dw=dw, db=db, mean=mean, rstd=rstd)
    if pb.fused:
        got.update(xo=xo[:, :C], da=da[:, :C])
    return got, bufs


def _knobs(i):
    """eps and out_scale of case number i: all four pairs come round."""
    return (1e-5, 1e-3)[i % 2], (1.0, 0.2)[(i // 2) % 2]


LN_CASES = [(combo, C, rows) for combo in rw.COMBOS for C in rw.WIDTHS for rows in rw.ROWS]


@pytest.mark.parametrize("combo,C,rows", LN_CASES, ids=[f"{c}-C{w}-r{r}" for c, w, r in LN_CASES])
def test_ln_matrix(combo, C, rows):
    """Every type combination x width x row count through ops._GroupLNScale."""
    eps, out_scale = _knobs(rw.WIDTHS.index(C) + rw.ROWS.index(rows))
    pb = rw.ln_problem(combo, rows, C, eps, out_scale)
    _check_ln(f"ops/{combo}-C{C}-r{rows}-eps{eps:g}-os{out_scale:g}", pb, _run_ops(pb))


FUSED_CASES = [(combo, C, rows) for combo in rw.MIXED for C in rw.WIDTHS for rows in (9, 513)]


@pytest.mark.parametrize("combo,C,rows", FUSED_CASES, ids=[f"{c}-C{w}-r{r}" for c, w, r in FUSED_CASES])
def test_add_ln_matrix(combo, C, rows):
    """The add + LN fusion through ops.add_layer_norm at the same widths, both output dtypes:
    xo = x + a, y, the stream's and the branch's gradients, dw / db."""
    eps, _ = _knobs(rw.WIDTHS.index(C))
    pb = rw.ln_problem(combo, rows, C, eps, 1.0, fused=True)
    _check_ln(f"ops/{combo}+add-C{C}-r{rows}-eps{eps:g}-os1", pb, _run_ops(pb))


STRIDED = [(combo, fused) for combo in rw.COMBOS for fused in (False, True) if not fused or combo in rw.MIXED]
STRIDED_CASES = [(combo, fused, C) for combo, fused in STRIDED for C in rw.WIDTHS]


@pytest.mark.parametrize("combo,fused,C", STRIDED_CASES, ids=[f"{c}{'+add' if f else ''}-C{w}" for c, f, w in STRIDED_CASES])
def test_ln_strided(combo, fused, C):
    """dta_ln_fwd / dta_ln_bwd with x, y, dy, dx, res, xo, dres and dx16 each on a row stride of
    its own (C + 8, C + 16, ...): the results as for packed rows, the gaps untouched."""
    eps, out_scale = _knobs(rw.WIDTHS.index(C) + 1)
    pb = rw.ln_problem(combo, 37, C, eps, out_scale, fused=fused, seed=1)
    got, bufs = _run_direct(pb)
    _gaps_untouched(bufs, C)
    _check_ln(f"abi/{combo}{'+add' if fused else ''}-C{C}-r37-eps{eps:g}-os{pb.out_scale:g}", pb, got)
    # packed rows through the same entry points: bit for bit the same results
    packed, _ = _run_direct(pb, pad=0)
    for name in got:
        assert torch.equal(got[name], packed[name]), name


@functools.lru_cache(maxsize=None)
def _base():
    return torch.randn(4099, 8192, generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("combo", ["f32", "bf16", "f32-bf16"])
@pytest.mark.parametrize("rows", [37, 4099])
@pytest.mark.parametrize("C", [1024, 3072, 8192])
def test_ln_every_row_counted_once(C, rows, combo):
    """dy zero but for one row r: dw = out_scale dy_r xhat_r and db = out_scale dy_r, so a row
    the backward skips or counts twice shows at full size, and every other row of dx is exactly
    zero.  CHB 1, 2, 4; 37 rows (5 workgroups, 7 or 8 rows each) and 4099 (the 512-workgroup cap
    binds, 8 or 9 rows each)."""
    lib = _lib.load()
    xdt, ydt = rw.COMBOS[combo]
    eps, out_scale = rw.f32(1e-5), rw.f32(0.2)
    x = (_base()[:rows, :C] * 2 + 0.5).to(xdt).contiguous()
    g = torch.Generator().manual_seed(C + rows)
    w = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    b = torch.zeros(C, device=DEV)
    xg = x.to(DEV)
    y = torch.empty(rows, C, dtype=ydt, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    pb = type("P", (), dict(combo=combo, rows=rows, C=C, eps=eps, out_scale=out_scale))
    _lib.check(lib.dta_ln_fwd(_ln_args(pb, x=xg.data_ptr(), x_stride=C, y=y.data_ptr(), y_stride=C, w=w.data_ptr(),
                                       b=b.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr()), _stream()))
    dy = torch.zeros(rows, C, dtype=ydt, device=DEV)
    dx = torch.empty(rows, C, dtype=xdt, device=DEV)
    part = torch.empty(lib.dta_ln_bwd_workspace_bytes(rows, C) // 4, device=DEV)
    targets = rw.single_row_targets(rows, C)
    assert len(targets) >= (4 if rows == 37 else 5)
    for r in targets:
        dyr = torch.randn(C, generator=g).to(ydt)
        dy[r] = dyr.to(DEV)
        dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        _lib.check(lib.dta_ln_bwd(_ln_args(pb, x=xg.data_ptr(), x_stride=C, w=w.data_ptr(), mean=mean.data_ptr(),
                                           rstd=rstd.data_ptr(), dy=dy.data_ptr(), dy_stride=C, dx=dx.data_ptr(), dx_stride=C,
                                           dw=dw.data_ptr(), db=db.data_ptr(), partial=part.data_ptr()), _stream()))
        xr = x[r].double()
        xh = (xr - xr.mean()) / (xr.var(unbiased=False) + eps).sqrt()
        assert rw.vec_err(dw, out_scale * dyr.double() * xh) < TOL[F32], (r, "dw")
        assert rw.vec_err(db, out_scale * dyr.double()) < TOL[F32], (r, "db")
        assert dx[r].abs().max() > 0
        dx[r] = 0
        assert not dx.any(), (r, "dx of a row whose dy is zero")
        dy[r] = 0


@pytest.mark.parametrize("combo", ["f32", "bf16", "f16", "f32-bf16", "f32-f16"])
def test_ln_dw_db_are_added_into(combo):
    """C = 3072 (CHB 2), 513 rows.  With a workspace two runs are bitwise equal and prefilled
    dw / db come back as prefill + the from-zero result, bitwise (ln_bwd_reduce adds one fp32
    total per column).  Without one (partial == NULL) the partials go in by atomics: against
    fp64 at fp32's bar, from zero and onto the prefill -- not reproducible by design."""
    C = 3072
    pb = rw.ln_problem(combo, 513, C, 1e-5, 0.2, seed=2)
    first, _ = _run_direct(pb, pad=0)
    again, _ = _run_direct(pb, pad=0)
    for name in first:
        assert torch.equal(first[name], again[name]), name
    g = torch.Generator().manual_seed(5)
    pre = (torch.randn(C, generator=g).to(DEV) * 10, torch.randn(C, generator=g).to(DEV) * 10)
    onto, _ = _run_direct(pb, pad=0, prefill=pre)
    assert torch.equal(onto["dw"], pre[0] + first["dw"]) and torch.equal(onto["db"], pre[1] + first["db"])
    assert torch.equal(onto["dx"], first["dx"])
    atom, _ = _run_direct(pb, pad=0, partial=False)
    assert rw.vec_err(atom["dw"], pb.oracle["dw"]) < TOL[F32] and rw.vec_err(atom["db"], pb.oracle["db"]) < TOL[F32]
    assert torch.equal(atom["dx"], first["dx"])
    atom, _ = _run_direct(pb, pad=0, partial=False, prefill=pre)
    assert rw.vec_err(atom["dw"], pb.oracle["dw"] + pre[0].double().cpu()) < TOL[F32]
    assert rw.vec_err(atom["db"], pb.oracle["db"] + pre[1].double().cpu()) < TOL[F32]


def test_ln_rejections():
    """What the entry points refuse is refused before anything launches: a width that is no
    multiple of 8 or beyond 8192, a row stride that is no multiple of 8, a 16-bit x with an
    io dtype, the fusion without one; RoPE below head size 8."""
    lib = _lib.load()
    x, y, w, b, m, r = (torch.zeros(4, 64, device=DEV) for _ in range(6))
    p = x.data_ptr()

    def fwd(**kw):
        base = dict(dtype=_lib.DTA_F32, rows=4, C=64, eps=1e-5, out_scale=1.0, x=p, x_stride=64, y=y.data_ptr(), y_stride=64,
                    w=w.data_ptr(), b=b.data_ptr(), mean=m.data_ptr(), rstd=r.data_ptr())
        base.update(kw)
        return lib.dta_ln_fwd(_lib.LnArgs(**base), _stream())

    assert fwd() == 0                    # the accepted call the refused ones are one step away from
    for kw in (dict(C=12, x_stride=16, y_stride=16), dict(C=8200, x_stride=8200, y_stride=8200), dict(x_stride=68),
               dict(y_stride=68), dict(dtype=_lib.DTA_BF16, io_dtype=2), dict(io_dtype=3), dict(res=p, res_stride=64, xo=p, xo_stride=64),
               dict(w=None), dict(x=p + 4)):
        assert fwd(**kw) != 0, kw
    ra = _lib.RopeArgs(_lib.DTA_F32, 1, 2, 1, 1, 4, 0, 0, _lib.DtaTensor(p, 8, 4, 4, 4), _lib.DtaTensor(p, 8, 4, 4, 4), p)
    assert lib.dta_rope(ra, _stream()) != 0
    torch.cuda.synchronize()


# ============================================================================= RoPE ===
ROPE_COMBOS = {"f32": (F32, F32), "bf16": (BF16, BF16), "f16": (F16, F16), "f32-bf16": (F32, BF16), "f32-f16": (F32, F16)}
ROPE_HN = [(1, 1), (3, 1), (6, 3), (5, 7)]
ROPE_HS = [8, 64, 96, 256]            # 8: the smallest head size dta_rope accepts
ROPE_T = [1, 17, 130]


@functools.lru_cache(maxsize=None)
def _freqs(hs, T):
    fc = orc.precompute_freqs_cis(hs, T)
    return fc, torch.view_as_real(fc).contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def _rope_ref(B, T, H, N, hs, inverse):
    src = rw.rope_source(B, T, H, N, hs)
    return src, rw.rope64(src, _freqs(hs, T)[0], inverse)


def _view5(t, strided, dtype):
    """``t`` (B, T, H, N, hs) on the GPU in ``dtype``: packed, or a slice of a wider buffer of
    SENTINEL (one more head, one more branch, 8 more columns; the slice starts at head 1).
    Returns (view, buffer)."""
    B, T, H, N, hs = t.shape
    if not strided:
        v = t.to(dtype).to(DEV).contiguous()
        return v, v
    buf = torch.full((B, T, H + 1, N + 1, hs + 8), SENTINEL, dtype=dtype, device=DEV)
    v = buf[:, :, 1:, :N, :hs]
    v.copy_(t.to(dtype))
    return v, buf


def _rope(src, dst, table, inverse):
    B, T, H, N, hs = src.shape
    ra = _lib.RopeArgs(_lib.dtype_code(dst.dtype), B, T, H, N, hs, int(inverse), int(src.dtype == F32 and dst.dtype != F32),
                       _lib.tensor5(src), _lib.tensor5(dst), table.data_ptr())
    _lib.check(_lib.load().dta_rope(ra, _stream()))


def _outside_untouched(buf, view_of, before):
    """Nothing but the view's own elements of ``buf`` changed."""
    after = buf.clone()
    view_of(after).copy_(view_of(before))
    assert torch.equal(after, before), "written outside the view"


def _rows_err(got, ref):
    """Row-wise error of a (B, T, ...) tensor: one row per (b, t)."""
    B, T = ref.shape[:2]
    return rw.row_errors(got.double().cpu().reshape(B * T, -1), ref.reshape(B * T, -1))[0]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("strided", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("combo", list(ROPE_COMBOS))
def test_rope_matrix(combo, strided, inverse):
    """dta_rope over (H, N) x head size x T: every row (b, t) of the result against fp64."""
    sdt, ddt = ROPE_COMBOS[combo]
    worst = (-1.0, ())
    for H, N in ROPE_HN:
        for hs in ROPE_HS:
            for T in ROPE_T:
                B = 2 if T < 100 else 1
                src64, ref = _rope_ref(B, T, H, N, hs, inverse)
                src, sbuf = _view5(src64, strided, sdt)
                dst, dbuf = _view5(torch.zeros_like(src64), strided, ddt)
                s0, d0 = sbuf.clone(), dbuf.clone()
                _rope(src, dst, _freqs(hs, T)[1], inverse)
                torch.cuda.synchronize()
                assert torch.equal(sbuf, s0), "the source was written"
                if strided:
                    _outside_untouched(dbuf, lambda b: b[:, :, 1:, :N, :hs], d0)
                e = _rows_err(dst, ref).max().item()
                assert e < rw.ROPE_BAR[ddt], (H, N, hs, T, e)
                worst = max(worst, (e, (H, N, hs, T)))
    print(combo, strided, inverse, "worst row", worst)


@pytest.mark.parametrize("combo", list(ROPE_COMBOS))
def test_rope_inverse_undoes_forward(combo):
    """inverse(forward(x)) = x to the dtype's rounding: two roundings, the first of values up to
    sqrt(2) x the row's maximum (2.4 unit roundoffs in all; the bar is twice one rounding's)."""
    sdt, ddt = ROPE_COMBOS[combo]
    for (H, N), hs, T in [((5, 7), 96, 130), ((6, 3), 8, 17), ((3, 1), 256, 130)]:
        src64, _ = _rope_ref(1, T, H, N, hs, False)
        src, _ = _view5(src64, False, sdt)
        mid, back = torch.empty(src.shape, dtype=ddt, device=DEV), torch.empty(src.shape, dtype=ddt, device=DEV)
        _rope(src, mid, _freqs(hs, T)[1], False)
        _rope(mid, back, _freqs(hs, T)[1], True)
        torch.cuda.synchronize()
        assert _rows_err(back, src64).max().item() < 2 * rw.ROPE_BAR[ddt], (H, N, hs, T)


def test_rope_grid_stride_wraps():
    """T = 16400, H = 16, N = 2, hs = 64, bf16: 16400 x 256 items, over the 16384 x 256 of one
    trip, so the last 16 rows are the loop's second trip.  Sampled rows: the first, the last and
    those on either side of the wrap."""
    T, H, N, hs = 16400, 16, 2, 64
    assert T * H * N * (hs // 8) > GRID_CAP and GRID_CAP // (H * N * hs // 8) == 16384
    rows = [0, 1, 16382, 16383, 16384, 16385, T - 2, T - 1]
    src = (torch.randint(-256, 257, (1, T, H, N, hs), device=DEV, generator=torch.Generator(DEV).manual_seed(3)) / 64).to(BF16)
    dst = torch.full(src.shape, SENTINEL, dtype=BF16, device=DEV)
    fc, table = _freqs(hs, T)
    _rope(src, dst, table, False)
    torch.cuda.synchronize()
    ref = rw.rope64(src[:, rows].cpu().double(), fc[rows])
    assert _rows_err(dst[:, rows], ref).max().item() < rw.ROPE_BAR[BF16]
    assert not (dst == SENTINEL).all(-1).any(), "a (row, head, branch) was left unwritten"


# =========================================================================== SwiGLU ===
def _swiglu(dtype, rows, n, a, b, out=None, dout=None, da=None, db=None, dbias=None):
    """dta_swiglu_fwd (``out``) or dta_swiglu_bwd on 2-d views with unit column stride."""
    lib = _lib.load()

    def ps(t):
        if t is None:
            return None, 0
        assert t.shape == (rows, n) and t.stride(1) == 1 and t.dtype == dtype
        return t.data_ptr(), t.stride(0)

    work = None
    if dbias is not None:
        work = torch.empty(lib.dta_swiglu_bwd_workspace_bytes(rows, n) // 4, device=DEV)
    sa = _lib.SwigluArgs(_lib.dtype_code(dtype), rows, n, *ps(a), *ps(b), *ps(out), *ps(dout), *ps(da), *ps(db),
                         _lib.ptr(dbias), _lib.ptr(work))
    _lib.check((lib.dta_swiglu_fwd if out is not None else lib.dta_swiglu_bwd)(sa, _stream()))


def _swiglu_layout(layout, dtype, rows, n, a, b, d):
    """The operands of one SwiGLU case on the GPU: name -> (rows, n) view, and the buffers
    to check for writes outside the views.  "halves": a | b and da | db are the column halves
    of packed (rows, 2n) buffers (the packed projection's layout); "strided": every operand a
    buffer of its own with a row stride beyond n, SENTINEL in the gaps."""
    if layout == "halves":
        y2 = torch.cat([a, b], 1).to(DEV)
        dy2 = torch.full((rows, 2 * n), SENTINEL, dtype=dtype, device=DEV)
        v = dict(a=y2[:, :n], b=y2[:, n:], d=d.to(DEV), out=torch.empty(rows, n, dtype=dtype, device=DEV),
                 da=dy2[:, :n], db=dy2[:, n:])
        return v, {}
    bufs = {k: _buf(t, rows, n, n + 8 * (i + 1), dtype) for i, (k, t) in
            enumerate((("a", a), ("b", b), ("d", d), ("out", None), ("da", None), ("db", None)))}
    return {k: t[:, :n] for k, t in bufs.items()}, bufs


@pytest.mark.parametrize("layout", ["halves", "strided"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_swiglu_tails(dtype, layout):
    """a drawn from {0, +-1e-4, +-10, +-20, +-87, +-89, +-100, +-1e4} (clipped to the dtype's
    range) among random data: where __expf(-a) underflows, saturates the sigmoid or overflows,
    every output is finite and matches fp64 element by element; the bias pass stores the same
    dA | dB bit for bit."""
    rows, n = 33, 520
    pb = rw.swiglu_problem(dtype, rows, n)
    v, bufs = _swiglu_layout(layout, dtype, rows, n, pb.a, pb.b, pb.d)
    _swiglu(dtype, rows, n, v["a"], v["b"], out=v["out"])
    _swiglu(dtype, rows, n, v["a"], v["b"], dout=v["d"], da=v["da"], db=v["db"])
    torch.cuda.synchronize()
    _gaps_untouched(bufs, n)
    plain = {k: v[k].clone() for k in ("da", "db")}
    for name in ("out", "da", "db"):
        assert torch.isfinite(v[name]).all(), name
        e = rw.elem_err(v[name].float(), pb.oracle[name], pb.aux[name], dtype)
        print(rw.NAME[dtype], layout, name, f"{e:.3g}")
        assert e < TOL[dtype], (name, e)
    dbias = torch.full((2 * n,), SENTINEL, device=DEV)
    v["da"].fill_(SENTINEL)
    v["db"].fill_(SENTINEL)
    _swiglu(dtype, rows, n, v["a"], v["b"], dout=v["d"], da=v["da"], db=v["db"], dbias=dbias)
    torch.cuda.synchronize()
    _gaps_untouched(bufs, n)
    assert torch.equal(v["da"], plain["da"]) and torch.equal(v["db"], plain["db"])
    ref = torch.cat([plain["da"].double().sum(0), plain["db"].double().sum(0)])
    assert torch.isfinite(dbias).all() and rw.vec_err(dbias, ref) < 1e-5


BIAS_ROWS = [1, 127, 128, 129, 2048, 2049, 4097]       # row blocks 1, 1, 1, 2, 16, 17, 33 against the 16 runs


@pytest.mark.parametrize("n", [64, 2056])
@pytest.mark.parametrize("rows", BIAS_ROWS)
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_swiglu_bias_pass_row_blocks(dtype, rows, n):
    """The bias pass's two-stage reduce at row-block counts that fill one of its 16 runs, two,
    all sixteen evenly, nine unevenly (2, ..., 2, 1) and eleven (3 each): dA | dB bitwise equal
    to the plain backward's, dbias against the fp64 column sums of the stored dA | dB."""
    gen = torch.Generator(DEV).manual_seed(rows + n)
    y2 = (torch.randn(rows, 2 * n, device=DEV, generator=gen) * 2).to(dtype)
    d = torch.randn(rows, n, device=DEV, generator=gen).to(dtype)
    ref2, dy2 = torch.empty_like(y2), torch.full_like(y2, SENTINEL)
    _swiglu(dtype, rows, n, y2[:, :n], y2[:, n:], dout=d, da=ref2[:, :n], db=ref2[:, n:])
    dbias = torch.full((2 * n,), SENTINEL, device=DEV)
    _swiglu(dtype, rows, n, y2[:, :n], y2[:, n:], dout=d, da=dy2[:, :n], db=dy2[:, n:], dbias=dbias)
    torch.cuda.synchronize()
    assert torch.equal(dy2, ref2)
    assert rw.vec_err(dbias, ref2.double().sum(0)) < 1e-5


def test_swiglu_grid_stride_wraps():
    """16321 rows x 2056 columns, bf16: 16321 x 257 items, just over one trip's 16384 x 256; the
    wrap falls inside row 16320.  The rows on either side of it, the first and the last against
    fp64; the packed halves layout."""
    rows, n = 16321, 2056
    assert (rows - 1) * (n // 8) < GRID_CAP < rows * (n // 8)
    gen = torch.Generator(DEV).manual_seed(9)
    y2 = (torch.randn(rows, 2 * n, device=DEV, generator=gen) * 3).to(BF16)
    out = torch.full((rows, n), SENTINEL, dtype=BF16, device=DEV)
    _swiglu(BF16, rows, n, y2[:, :n], y2[:, n:], out=out)
    torch.cuda.synchronize()
    sample = [0, 1, GRID_CAP // (n // 8) - 1, GRID_CAP // (n // 8), rows - 1]
    assert sample[3] == rows - 1 and sample[2] == rows - 2
    a, b = y2[sample, :n].double().cpu(), y2[sample, n:].double().cpu()
    ref = torch.nn.functional.silu(a) * b
    assert rw.elem_err(out[sample].float(), ref, torch.zeros_like(ref), BF16) < TOL[BF16]
    assert not (out == SENTINEL).all(-1).any()


# ================================================================= cast_f32, accumulate ===
def _cast(src, dst):
    B, T, H, N, hs = dst.shape
    _lib.check(_lib.load().dta_cast_f32(_lib.dtype_code(dst.dtype), B, T, H, N, hs, src.data_ptr(), _lib.tensor5(dst), _stream()))


def _assert_same_bits(got, want, src):
    """Bitwise equality with torch's single round-to-nearest-even; a mismatch names the values."""
    same = got.view(torch.int16 if got.element_size() == 2 else torch.int32) == \
        want.view(torch.int16 if want.element_size() == 2 else torch.int32)
    if not same.all():
        i = torch.nonzero(~same.flatten())[:8].flatten()
        raise AssertionError(f"cast differs from torch at fp32 values {src.flatten()[i].tolist()}: "
                             f"kernel {got.flatten()[i].tolist()}, torch {want.flatten()[i].tolist()}")


CAST_SPECIALS = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,   # ties, both ways
                 1.0 + 2.0 ** -8 + 2.0 ** -20, 65504.0, 65519.9, 65520.0, 70000.0, -70000.0, 3.0e38, 3.4e38, float("inf"),
                 -float("inf"), 6.0e-5, 6.1e-5, 5.96e-8, 2.98e-8, 2.99e-8, 1.0e-8, 1.0e-30, 1.2e-38, 1.0e-40, -1.0e-40]


@pytest.mark.parametrize("strided", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
def test_cast_f32(dtype, strided):
    """dta_cast_f32 into packed and strided 5-d destinations: bitwise torch's .to(dtype) (one
    round-to-nearest-even), ties, the fp16 overflow edge, subnormals and infinities included."""
    B, T, H, N, hs = 2, 5, 3, 2, 24
    g = torch.Generator().manual_seed(13)
    src = torch.randn(B, T, H, N, hs, generator=g) * 10.0 ** torch.randint(-6, 5, (B, T, H, N, 1), generator=g).float()
    src.view(-1)[:len(CAST_SPECIALS)] = torch.tensor(CAST_SPECIALS)
    src = src.to(DEV)
    dst, buf = _view5(torch.zeros(B, T, H, N, hs), strided, dtype)
    dst.fill_(SENTINEL)
    before = buf.clone()
    _cast(src, dst)
    torch.cuda.synchronize()
    if strided:
        _outside_untouched(buf, lambda b: b[:, :, 1:, :N, :hs], before)
    _assert_same_bits(dst.contiguous(), src.to(dtype), src)


def test_cast_f32_grid_stride_wraps():
    """(1, 16400, 16, 2, 64) into bf16: over one trip's 16384 x 256 items.  The whole tensor is
    compared on the GPU, the wrap's two sides with it."""
    B, T, H, N, hs = 1, 16400, 16, 2, 64
    assert B * T * H * N * hs // 8 > GRID_CAP
    src = torch.randn(B, T, H, N, hs, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    dst = torch.full(src.shape, SENTINEL, dtype=BF16, device=DEV)
    _cast(src, dst)
    torch.cuda.synchronize()
    for rows in (slice(0, 2), slice(16382, 16386), slice(T - 2, T)):
        _assert_same_bits(dst[:, rows].contiguous(), src[:, rows].to(BF16), src[:, rows])
    assert torch.equal(dst, src.to(BF16))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_accumulate_grid_stride_wraps(dtype):
    """n = 4096 x 256 x 8 + 2405: two blocks' worth beyond accumulate's 4096-block cap and a
    5-element scalar tail; bitwise torch's fp32 add of the upcast source."""
    n = 4096 * 256 * 8 + 2405
    assert (n + 7) // 8 > 4096 * 256 and n % 8 == 5
    gen = torch.Generator(DEV).manual_seed(6)
    g = torch.randn(n, device=DEV, generator=gen)
    d = torch.randn(n, device=DEV, generator=gen).to(dtype)
    ref = g + d.float()
    packing.accumulate(g, d)
    torch.cuda.synchronize()
    wrap = 4096 * 256 * 8
    for lo, hi in ((0, 16), (wrap - 16, wrap + 16), (n - 16, n)):
        assert torch.equal(g[lo:hi], ref[lo:hi]), (lo, hi)
    assert torch.equal(g, ref)
