"""Band-resolved parity of the training-path attention core (tests/_bands.py).

The other parity modules take ``rel_err`` over a whole tensor; under the causal mask its
denominator comes from the first rows, so the late rows -- a K/V ring that has wrapped many
times, the ragged last tile, softmax statistics carried over every tile, dK/dV summed over
branch groups -- could be wrong by a multiple of themselves unseen.  Here O, dQ, dK and dV of
``ops.diff_attention`` are compared with the fp64 oracle over bands of rows (octaves below 64,
then 64-row tiles) per batch, head and branch, and every dcoef entry against its head's largest.

Bars: the existing whole-tensor ``TOL`` first; then per tensor ``max(TOL, 2 x the worst band
error of the reference algorithm run in the kernel's dtype on the CPU)`` -- made of the oracle
and ``_bands.reference_algorithm`` only.  Blocks whose oracle is exactly zero (dQ of row 0, and
under dropout the rows that keep no key) are asserted to be those and nothing else, and the
kernel's values there are held under TOL of the tensor's oracle maximum.

Every case is B = 2: the smallest shapes at which the ring wraps several times and the tail
tile is ragged.  With DTA_BAND_ERRORS_JSON set, the figures of every case are written there
(profiles/band_errors.json is such a run).
"""
import contextlib
import functools
import json
import os

import pytest
import torch

import _bands
from test_gpu_parity import TOL
from test_gpu_plan_matrix import BF16, F16, F32, NAME, SEED, SIXTEEN, _assert_parity, _f32, _gpu, _problem, _switch

from differential_transformer_replication_amd import _lib, ops

pytestmark = pytest.mark.gpu

_REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _band_report():
    """With DTA_BAND_ERRORS_JSON set, every case's figures are written there."""
    yield
    path = os.environ.get("DTA_BAND_ERRORS_JSON")
    if path and _REPORT:
        margin = min((t["bar"] / t["kernel"], c, n) for c, ts in _REPORT.items() for n, t in ts.items() if t["kernel"] > 0)
        with open(path, "w") as fh:
            json.dump({"norm": "max|kernel - oracle| / max|oracle| over each block of (row band) x (batch, head[, branch]); "
                               "row bands [0,1) [1,2) [2,4) ... [32,64), then 64-row tiles, the last ragged; dcoef: "
                               "each entry over its head's largest oracle entry",
                       "bar": "max(TOL[dtype], 2 x yardstick): the reference algorithm in the case's dtype on the CPU "
                              "(tests/_bands.py reference_algorithm), its worst band against the same fp64 oracle",
                       "fields": "kernel: the kernels' worst band error; where: [[first row, end row], [b, h(, branch)]] "
                                 "of that band ([h, i] for dcoef); yardstick: the reference algorithm's worst band; "
                                 "step / yardstick_plain: the rounding step the path takes by design, which its "
                                 "yardstick emulates (reference_algorithm's option), and the worst band without it",
                       "smallest_bar_over_kernel": {"ratio": margin[0], "case": margin[1], "tensor": margin[2]},
                       "cases": _REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


@functools.lru_cache(maxsize=4)
def _yardstick(dtype, H, N, hs, T, rope, dv, p, seed, step=None):
    """The problem (inputs, fp64 oracle) and the reference algorithm's run on it, once for the
    cases that share them.  ``step``: a rounding step the path under test takes by design, named
    as reference_algorithm's option ("obr_f16")."""
    pb = _problem(dtype, H, N, hs, T, rope, dv, p, seed)
    opts = {step: True} if step else {}
    yard = _bands.reference_algorithm(pb.qkv, pb.coef, pb.do, H, N, hs, dv, dtype, pb.freqs_c, pb.masks, **opts)
    return pb, yard


def _expected_zero_blocks(pb):
    """name -> the (band, b, h[, i]) blocks whose oracle is exactly zero, from the problem alone:
    dQ_i of row 0 (one key: P = 1, dS = 0) and of a row whose every causal key is dropped (dP = 0);
    O of a row dropped in every branch; dV of a key no query keeps in any branch; dK never (a
    dropped element still carries -P delta)."""
    B, T, H, N, hs, dv = pb.dims
    bands = _bands.row_bands(T)
    gone = torch.zeros(B, T, H, N, dtype=torch.bool)
    unkept = torch.zeros(B, T, H, dtype=torch.bool)
    if pb.masks is not None:
        kept = (pb.masks > 0) & torch.tril(torch.ones(T, T, dtype=torch.bool))          # (B, H, N, Tq, Tk)
        gone = kept.sum(-1).eq(0).permute(0, 3, 1, 2)
        unkept = kept.sum((2, 3)).eq(0).permute(0, 2, 1)
    dq = gone.clone()
    dq[:, 0] = True

    def per_band(rows):
        return torch.stack([rows[:, lo:hi].all(1) for lo, hi in bands])

    return {"O": per_band(gone.all(-1)), "dQ": per_band(dq), "dK": torch.zeros(len(bands), B, H, N, dtype=torch.bool),
            "dV": per_band(unkept)}


def _band_case(case, dtype, H, N, hs, T, rope, dv=None, p=0.0, step=None):
    dv = 2 * hs if dv is None else dv
    assert ops.attention_supported(dtype, hs, N, dv)
    p = _f32(p)
    pb, plain = _yardstick(dtype, H, N, hs, T, rope, dv, p, SEED)
    yard = _yardstick(dtype, H, N, hs, T, rope, dv, p, SEED, step)[1] if step else plain
    got = _gpu(pb, p, SEED)
    tol = TOL[dtype]
    res = _bands.judge(got, (pb.out, pb.gx, pb.gc), yard, pb.dims, tol, plain if step else None)
    _REPORT[case] = {n: {"kernel": r.kernel, "where": r.where, "yardstick": r.yardstick, "bar": r.bar} for n, r in res.items()}
    if step:
        for n, r in res.items():
            _REPORT[case][n].update(step=step, yardstick_plain=r.plain)
    print(case, {n: f"{r.kernel:.3g} / {r.bar:.3g} (yardstick {r.yardstick:.3g}) at {r.where}" for n, r in res.items()})
    _assert_parity(pb, got, tol, case)                             # the whole-tensor bars, as everywhere
    want = _expected_zero_blocks(pb)
    if not p:
        assert want["dQ"][0].all() and not want["dQ"][1:].any()
    for name in ("O", "dQ", "dK", "dV"):
        assert torch.equal(res[name].zero, want[name]), f"{name}: zero-oracle blocks other than the expected ones"
        assert res[name].excess <= tol, (name, "in the zero-oracle blocks", res[name].excess)
    bad = {n: (r.kernel, r.where, r.bar) for n, r in res.items() if not r.kernel < r.bar}
    assert not bad, (case, bad)


def _id(dtype, H, N, hs, T, rope):
    return f"{NAME[dtype]}-H{H}-N{N}-hs{hs}-T{T}" + ("-rope" if rope else "")


# ======================================================= A. the default plans ===
SHAPES_A = [  # H, N, hs, T, rope
    (2, 2, 64, 1100, False), (1, 1, 64, 777, False), (1, 3, 32, 1500, True), (1, 2, 96, 700, True),
    (1, 2, 128, 520, False), (1, 4, 64, 520, False), (1, 2, 256, 330, False),
]
CASES_A = [(d, *s) for s in SHAPES_A for d in (F32, BF16, F16) if not (s[2] == 256 and d == F32)]


@pytest.mark.parametrize("dtype,H,N,hs,T,rope", CASES_A, ids=[_id(*c) for c in CASES_A])
def test_default_plans(dtype, H, N, hs, T, rope):
    _band_case("A/" + _id(dtype, H, N, hs, T, rope), dtype, H, N, hs, T, rope)


# ===================================== B. native 3- and 4-branch backward plans ===
CASES_B = [(d, *s) for s in [(1, 3, 128, 520, True), (1, 4, 96, 520, False), (2, 3, 64, 520, True)] for d in SIXTEEN]


@pytest.mark.parametrize("dtype,H,N,hs,T,rope", CASES_B, ids=[_id(*c) for c in CASES_B])
def test_native_backward_plans(dtype, H, N, hs, T, rope):
    code = _lib.dtype_code(dtype)
    with ops.bwd_group_caps(4, 4):
        assert _lib.load().dta_attn_bwd_dkdv_groups(code, hs, N, 2 * hs, 4) == 1
        _band_case("B/caps44-" + _id(dtype, H, N, hs, T, rope), dtype, H, N, hs, T, rope)


# ============================================== C. the other storage paths ===
CASES_C = [(d, *s, path) for s in [(2, 3, 64, 520, False), (2, 2, 64, 520, False)] for d in SIXTEEN
           for path in ("lse_c-off", "dv_f32-off", "obr-f16")]


@pytest.mark.parametrize("dtype,H,N,hs,T,rope,path", CASES_C, ids=[_id(*c[:-1]) + "-" + c[-1] for c in CASES_C])
def test_storage_paths(dtype, H, N, hs, T, rope, path, monkeypatch):
    """Without the |c_i| fold workspace; without the fp32 dV workspace (N = 3 at head size 64
    runs dK/dV in groups, the later ones read-add-store the 16-bit dV); O_i stored as fp16.
    The last is a rounding step the reference algorithm does not take -- delta_i = <dO, O_i>
    from an fp16 O_i -- and against the plain yardstick it put dQ of row 1 of one (b, h, branch)
    at 2.39e-2 over the 2e-2 bar (fp16, N 3).  Its yardstick therefore emulates exactly that
    step (reference_algorithm's obr_f16: 1.24e-2 on that same block, bar 2.48e-2); the factor
    stays 2 and the report carries both yardsticks."""
    ctx = contextlib.nullcontext()
    if path == "lse_c-off":
        ctx = _switch(ops._LSE_C_WORKSPACE, False)
    elif path == "dv_f32-off":
        if N == 3:
            assert _lib.load().dta_attn_bwd_dkdv_groups(_lib.dtype_code(dtype), hs, N, 2 * hs, 0) > 1
        ctx = _switch(ops._DV_F32_WORKSPACE, False)
    else:
        monkeypatch.setenv("DTA_OBR_F16", "1")
        assert ops._obr_dtype(dtype) == F16
    with ctx:
        _band_case(f"C/{path}-" + _id(dtype, H, N, hs, T, rope), dtype, H, N, hs, T, rope,
                   step="obr_f16" if path == "obr-f16" else None)


# =================================================================== D. dropout ===
CASES_D = [(d, *s) for s in [(2, 2, 64, 520, False), (1, 3, 64, 520, True)] for d in SIXTEEN]


@pytest.mark.parametrize("dtype,H,N,hs,T,rope", CASES_D, ids=[_id(*c) for c in CASES_D])
def test_dropout(dtype, H, N, hs, T, rope):
    """p = 0.2: the oracle and the yardstick apply the same restated masks."""
    _band_case("D/p0.2-" + _id(dtype, H, N, hs, T, rope), dtype, H, N, hs, T, rope, p=0.2)


# =========================================================== E. a control width ===
def test_control_width():
    """N = 1, dv = hs (control.py's standard attention on the fused kernels)."""
    _band_case("E/control-" + _id(BF16, 2, 1, 128, 520, False), BF16, 2, 1, 128, 520, False, dv=128)
