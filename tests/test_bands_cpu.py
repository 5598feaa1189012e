"""The band-resolved norm (tests/_bands.py) must be able to fail where ``rel_err`` cannot, and
its yardstick -- the reference algorithm run in the kernel's dtype -- must hold without any
kernel: both shown on the CPU with the fp64 oracle alone.
"""
import functools
import types

import pytest
import torch

import _bands
from conftest import rel_err
from oracle import diffattn_oracle as orc
from test_gpu_parity import TOL, _oracle_core

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
LONG = (2, 1, 2, 64, 1100, False)         # B, H, N, hs, T, rope: the suite's long shape
ROPE = (1, 2, 3, 32, 200, True)


@functools.lru_cache(maxsize=None)
def _case(dtype, B, H, N, hs, T, rope):
    """Inputs quantised to ``dtype``, the fp64 oracle's forward and backward, and the reference
    algorithm's in ``dtype``."""
    dv = 2 * hs
    g = torch.Generator().manual_seed(1000 * H + 100 * N + hs + T)
    qkv = torch.randn(B, T, 2 * H * N * hs + H * dv, generator=g).to(dtype)
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    do = torch.randn(B, T, H * dv, generator=g).to(dtype)
    freqs_c = orc.precompute_freqs_cis(hs, max(T, 8)) if rope else None
    x64 = qkv.double().requires_grad_(True)
    c64 = coef.double().requires_grad_(True)
    ref = _oracle_core(x64, c64, H, N, hs, freqs_c)
    ref.backward(do.double())
    yard = _bands.reference_algorithm(qkv, coef, do, H, N, hs, dv, dtype, freqs_c)
    dims = (B, T, H, N, hs, dv)
    return types.SimpleNamespace(oracle=(ref.detach(), x64.grad, c64.grad), yard=yard, dims=dims,
                                 ref=_bands.tensors(ref.detach(), x64.grad, H, N, hs, dv))


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129, 1100])
def test_row_bands_cover_every_row_once(T):
    bands = _bands.row_bands(T)
    assert [r for lo, hi in bands for r in range(lo, hi)] == list(range(T))
    assert all(lo < hi for lo, hi in bands)
    octaves = [(0, 1), (1, 2), (2, 4), (4, 8), (8, 16), (16, 32), (32, 64)]
    assert bands[:7] == [(lo, min(hi, T)) for lo, hi in octaves if lo < T]
    assert all(lo % 64 == 0 and hi - lo == 64 for lo, hi in bands[7:-1])
    assert bands[-1][1] == T


def test_sampled_bands_merge_thin_bands():
    rows = [0, 1, 31, 32, 63, 64, 127, 128, 255, 700, 1099]
    got = _bands.sampled_bands(rows, 1100)
    assert [rows[lo:hi] for lo, hi in got] == [[0, 1], [31, 32, 63], [64, 127], [128, 255], [700, 1099]]
    assert _bands.sampled_bands([5], 64) == [(0, 1)]
    # dQ: row 0 (an exactly zero oracle) stays in its band without counting towards the two rows
    got = _bands.sampled_bands(rows, 1100, uncounted=(0,))
    assert [rows[lo:hi] for lo, hi in got] == [[0, 1, 31], [32, 63], [64, 127], [128, 255], [700, 1099]]
    assert [rows[lo:hi] for lo, hi in _bands.sampled_bands(rows[:-1], 1100)][-1] == [128, 255, 700]


# name, rows of the plant, the branch it is confined to (None: every group)
PLANTS = [("O", (1024, 1088), None), ("dQ", (1024, 1088), None), ("dK", (1024, 1088), None), ("dV", (1024, 1088), None),
          ("dV", (1088, 1100), None), ("dK", (1024, 1088), 1)]


@pytest.mark.parametrize("name,rows,branch", PLANTS, ids=[f"{n}-{r[0]}-{'all' if b is None else b}" for n, r, b in PLANTS])
def test_planted_late_error_passes_rel_err_and_fails_its_band(name, rows, branch):
    """1e-2 of the tensor's largest value added to one late band: the whole-tensor norm reads
    1e-2 and passes the 2e-2 bf16 bar, the band's own norm is far over the band bar (which is
    made of the bf16 reference algorithm's worst band, the widest bar of the three dtypes)."""
    cs = _case(BF16, *LONG)
    ref = cs.ref[name]
    got = ref.clone()
    top = ref.abs().max().item()
    if branch is None:
        got[:, rows[0]:rows[1]] += 1e-2 * top
    else:
        got[:, rows[0]:rows[1], :, branch] += 1e-2 * top
    assert rel_err(got, ref) < TOL[BF16]
    yard = _bands.tensors(cs.yard[0], cs.yard[1], *cs.dims[2:])
    y_w = _bands.band_errors(yard[name], ref, 1, _bands.GROUPS[name])[0].max().item()
    bar = _bands.bar(TOL[BF16], y_w)
    assert TOL[BF16] <= bar < 4e-2
    err, _ = _bands.band_errors(got, ref, 1, _bands.GROUPS[name])
    bands = _bands.row_bands(LONG[4])
    hit = bands.index(rows)
    assert (err[hit] > bar).all() if branch is None else (err[hit, ..., branch] > bar).all()
    clean = err.clone()
    if branch is None:
        clean[hit] = 0
    else:
        clean[hit, ..., branch] = 0
    assert (clean == 0).all(), "the error must be reported in the planted blocks only"
    w, w_rows, w_grp = _bands.worst(err, T=LONG[4])
    assert w > bar and w_rows == list(rows) and (branch is None or w_grp[-1] == branch)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", [LONG, ROPE], ids=["N2-hs64-T1100", "N3-hs32-T200-rope"])
def test_yardstick_holds_without_a_kernel(dtype, shape):
    """The reference algorithm in ``dtype`` against fp64, per band: under TOL[dtype] on every
    tensor (so a bar of max(TOL, 2 x it) is below 2 TOL), and the only blocks whose oracle is
    exactly zero are dQ's row 0 (one key: P = 1, dS = 0), one per (b, h, branch)."""
    cs = _case(dtype, *shape)
    B, T, H, N, hs, dv = cs.dims
    res = _bands.judge(cs.yard, cs.oracle, cs.yard, cs.dims, TOL[dtype])
    print({k: f"{v.yardstick:.3g}" for k, v in res.items()})
    for name, r in res.items():
        assert r.yardstick < TOL[dtype], (name, r.yardstick)
        assert r.bar == max(TOL[dtype], 2 * r.yardstick)
        assert r.excess < TOL[dtype], name
    for name in ("O", "dK", "dV"):
        assert not res[name].zero.any(), name
    zero = res["dQ"].zero
    assert zero.shape == (len(_bands.row_bands(T)), B, H, N)
    assert zero[0].all() and not zero[1:].any()


def test_packed_p_step_moves_only_nearly_one_hot_rows():
    """reference_algorithm's ``packed_p`` (P packed to the dtype against the first key tile's
    maximum, the row sum from the fp32 P): in fp32 it is the plain algorithm; in bf16 at unit-normal
    inputs it stays within the plain algorithm's own band errors; and in a row whose softmax has
    grown past its first tile onto one key (p_top about 1 - 4e-3 with a packed P of 2^growth, not
    1) it moves dQ by the rounding of that P over (1 - p_top), which the plain algorithm does not
    see -- the one place where the two yardsticks part."""
    B, H, N, hs, T, _ = LONG
    dv = 2 * hs
    g = torch.Generator().manual_seed(7)
    T = 130
    qkv = torch.randn(1, T, 2 * H * N * hs + H * dv, generator=g)
    coef = torch.tensor([[1.0, -0.3]])
    do = torch.zeros(1, T, H * dv)
    do[0, T - 1] = torch.randn(dv, generator=g)
    args = (H, N, hs, dv)
    plain = _bands.reference_algorithm(qkv, coef, do, *args, F32)
    step = _bands.reference_algorithm(qkv, coef, do, *args, F32, packed_p=True)
    for a, b in zip(plain, step):
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()
    cs = _case(BF16, *LONG)
    B, T2 = cs.dims[:2]
    g = torch.Generator().manual_seed(1000 * H + 100 * N + hs + T2)          # _case's inputs again
    x = torch.randn(B, T2, 2 * H * N * hs + H * dv, generator=g).to(BF16)
    c = torch.randn(H, N, generator=g) * 0.5
    c[:, 0] = 1.0
    d_o = torch.randn(B, T2, H * dv, generator=g).to(BF16)
    res = _bands.judge(_bands.reference_algorithm(x, c, d_o, *args, BF16, packed_p=True), cs.oracle, cs.yard, cs.dims, TOL[BF16])
    assert all(r.kernel < r.bar for r in res.values()), {n: (r.kernel, r.bar) for n, r in res.items()}
    # the last row of branch 0 points at key 100 (outside the first tile): q = 13.1 k_100 / |k_100|,
    # a logit of about 13 nats against unit-normal rivals
    k100 = qkv[0, 100, H * N * hs:H * N * hs + hs].clone()
    qkv[0, T - 1, :hs] = k100 * 13.1 / k100.norm()
    qkv = qkv.to(BF16)
    do = do.to(BF16)
    x64, c64 = qkv.double().requires_grad_(True), coef.double().requires_grad_(True)
    _oracle_core(x64, c64, H, N, hs).backward(do.double())
    ref = x64.grad[0, T - 1, :hs]
    plain = _bands.reference_algorithm(qkv, coef, do, *args, BF16)[1][0, T - 1, :hs]
    step = _bands.reference_algorithm(qkv, coef, do, *args, BF16, packed_p=True)[1][0, T - 1, :hs]
    moved = (step - plain).abs().max().item() / ref.abs().max().item()
    print("nearly one-hot row: plain", ((plain - ref).abs().max() / ref.abs().max()).item(), "moved by", moved)
    assert moved > TOL[BF16]
