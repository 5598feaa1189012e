"""tests/_rowwise.py without a GPU: the per-row measure must fail where ``rel_err`` cannot, the
width list of the GPU matrix must reach every LN instantiation at both edges of its band, and
the yardsticks -- the plain fp32 algorithm on the planted rows -- must hold against the fp64
oracle on their own, so that no bar ends up testing nothing.
"""
import pytest
import torch

import _rowwise as rw
from conftest import rel_err

F32, BF16, F16 = rw.F32, rw.BF16, rw.F16


def test_width_list_hits_every_band_at_both_edges():
    """ch = ceil(C / 512) into {1, 2, 4, 8, 16} (ln_launch / ln_launch_mixed); backward
    CHB = (CH + 3) / 4.  The matrix's widths reach all five at the narrowest and the widest
    width of each, the backward's three CHB, and the model widths 2560 / 3072 / 4096 land in
    the band no test used to launch."""
    assert [rw.ln_band(C) for C in (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [rw.ln_band(C) for C in (48, 384, 768, 1024, 2048, 4104, 8192)] == [1, 1, 2, 2, 4, 16, 16]     # the earlier lists: no 8
    assert [rw.ln_band(C) for C in (2560, 3072, 4096)] == [8, 8, 8]
    assert [rw.ln_band(C) for C in (0, 4, 12, 8200, 16384)] == [None] * 5
    for band in rw.LN_BANDS:
        lo, hi = rw.band_edges(band)
        assert rw.ln_band(lo) == band and rw.ln_band(hi) == band
        assert rw.ln_band(lo - 8) != band and rw.ln_band(hi + 8) != band
        assert lo in rw.WIDTHS and hi in rw.WIDTHS, (band, lo, hi)
    assert {rw.ln_band(C) for C in rw.WIDTHS} == set(rw.LN_BANDS)
    assert {rw.ln_bwd_chb(C) for C in rw.WIDTHS} == {1, 2, 4}
    assert [rw.ln_bwd_chb(C) for C in (1024, 3072, 8192)] == [1, 2, 4]
    assert [rw.ln_bwd_ring(C) for C in (1024, 3072, 8192)] == [4, 2, 2]


def test_single_row_targets():
    """37 rows: 5 workgroups, rows b, b + 5, ...; workgroups 0-1 own 8 rows, 2-4 own 7 (a ring
    slot left part filled at either ring size).  4099 rows: the 512-workgroup cap binds, 8 or 9
    rows each."""
    assert rw.ln_bwd_blocks(37) == 5 and rw.ln_bwd_blocks(4099) == 512
    assert rw.single_row_targets(37, 1024) == [0, 1, 5, 32, 36]         # 32: workgroup 2's 7th row
    assert rw.single_row_targets(37, 3072) == [0, 1, 5, 32, 36]
    assert rw.single_row_targets(4099, 1024) == [0, 1, 512, 4096, 4098]   # 4096: workgroup 0's 9th row
    assert rw.single_row_targets(4099, 8192) == [0, 1, 512, 4096, 4098]


def test_row_measure_fails_where_rel_err_passes():
    """A large-spread row's dx is a thousandth of its neighbours' (dx scales with rstd): wiped
    out entirely it moves ``rel_err`` by less than fp32's 1e-4, and the per-row measure by 1."""
    pb = rw.ln_problem("f32", 37, 1024, 1e-5, 0.2)
    dx = pb.oracle["dx"]
    row = 6                                    # scale 1e3
    assert pb.x[row].std() > 500
    bad = dx.clone()
    bad[row] = 0.0
    assert rel_err(bad, dx) < rw.TOL[F32]
    err, zero = rw.row_errors(bad, dx)
    assert err[row] == 1.0 and err.sum() == 1.0
    j = rw.judge_rows(bad, dx, pb.yard["dx"], rw.TOL[F32])
    assert j.where == row and [o[0] for o in j.over] == [row]
    # and the untouched tensor passes the same measure
    assert not rw.judge_rows(dx, dx, pb.yard["dx"], rw.TOL[F32]).over
    # the zero-dy row is exactly zero in the oracle and is reported as such, not as an error
    assert torch.equal(zero, rw.expected_zero_rows(pb, "dx"))
    bad = dx.clone()
    bad[pb.plant["zero_dy"]] = 1e-3 * dx.abs().max()
    assert rw.row_errors(bad, dx)[0].max() == 0 and rw.zero_row_excess(bad, dx) == pytest.approx(1e-3)


def test_dropped_row_of_dw_shows_only_with_one_nonzero_row():
    """5003 equal rows: one dropped from the column sum moves dw by about 1/sqrt(rows), under the
    16-bit bar the sums used to be judged at.  With dy zero but for one row it moves it by 1."""
    g = torch.Generator().manual_seed(0)
    terms = torch.randn(5003, 64, generator=g, dtype=torch.float64)
    full = terms.sum(0)
    assert rw.vec_err(full - terms[17], full) < rw.TOL[BF16]
    assert rw.vec_err(full - terms[17], full) > rw.TOL[F32]
    assert rw.vec_err(terms[17] - terms[17], terms[17]) == 1.0


CASES = [(combo, rows, C) for combo in rw.COMBOS for rows in (9, 513) for C in (8, 520, 3072, 8192)
         if not (rows == 513 and C in (8, 520))]


@pytest.mark.parametrize("combo,rows,C", CASES, ids=[f"{c}-r{r}-C{w}" for c, r, w in CASES])
def test_yardsticks_hold_on_the_planted_rows(combo, rows, C):
    """The plain fp32 algorithm on the scaled, offset and planted rows stays within 10 x TOL of
    the fp64 oracle in every row (most stay under TOL / 2, where the bar is TOL itself); dw, db,
    mean and rstd stay under fp32's TOL outright."""
    for fused in ((False, True) if combo in rw.MIXED else (False,)):
        pb = rw.ln_problem(combo, rows, C, 1e-5 if C % 16 else 1e-3, 0.2, fused=fused)
        res = rw.judge_ln(pb, {k: v for k, v in pb.yard.items()})
        tols = rw.ln_tols(combo)
        for name, r in res.items():
            assert not r.over, (name, r.over)
            assert r.yardstick < 10 * tols.get(name, rw.TOL[F32]), (name, r.yardstick)
            assert r.excess == 0.0, name
        for name in ("dx", "da", "xo"):
            if name in res:
                assert torch.equal(rw.row_errors(pb.yard[name].float(), pb.oracle[name])[1], rw.expected_zero_rows(pb, name))
        for name in ("dw", "db", "mean", "rstd"):
            assert res[name].yardstick < rw.TOL[F32], (name, res[name].yardstick)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_swiglu_oracle_is_finite_at_the_tails(dtype):
    """Every tail value survives the clip to the dtype's range and the fp64 reference is finite
    and representable there, so a non-finite kernel output is the kernel's."""
    pb = rw.swiglu_problem(dtype, 33, 520)
    vals = set(pb.a.double().flatten().tolist())
    for v in rw.SWIGLU_TAILS:
        q = torch.tensor(v).to(dtype).double().item()
        assert q in vals and -q in vals, v
    for name, t in pb.oracle.items():
        assert torch.isfinite(t).all() and torch.isfinite(t.to(dtype)).all(), name
        # the oracle rounded once to the dtype passes its own measure
        assert rw.elem_err(t.to(dtype), t, pb.aux[name], dtype) < rw.TOL[dtype]


def test_rope_reference_inverts():
    from oracle import diffattn_oracle as orc
    x = rw.rope_source(2, 17, 3, 2, 24)
    assert torch.equal(x, x.float().double()) and torch.equal(x, x.to(BF16).double()) and torch.equal(x, x.to(F16).double())
    fc = orc.precompute_freqs_cis(24, 17)
    y = rw.rope64(x, fc)
    assert y.shape == x.shape and rel_err(rw.rope64(y, fc, inverse=True), x) < 1e-6
    assert torch.equal(y[:, 0], x[:, 0])                     # position 0 rotates by nothing
    assert rel_err(y[0, :, 1, 1], orc.apply_rotary_emb(x[:1, :, 1, 1].float(), fc)[0]) < 1e-6
