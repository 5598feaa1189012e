"""CPU checks of the drop-in boundary: library exports, state_dict keys,
seeded-initialisation parity, reference state_dict loading, and that the
product path refuses to run anywhere but the HIP library (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Golden, ROOT, rel_err

import differential_transformer_replication_amd as dta
from differential_transformer_replication_amd import _lib
from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import Ndiff_transformer as ND
from differential_transformer_replication_amd import control as C


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "diffattn.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(dta_\w+)\s*\(", src, re.M)))


def test_header_matches_binding_list():
    assert sorted(_lib.EXPORTS) == _header_symbols()


def test_library_loads_and_exports():
    lib = _lib.load()
    for sym in _header_symbols():
        assert hasattr(lib, sym), sym
    assert lib.dta_abi_version() == _lib.ABI_VERSION
    assert b"unsupported" in lib.dta_error_string(-2)
    # host-only queries (no GPU needed)
    assert _lib.supported(torch.bfloat16, 64, 2, 128)
    assert _lib.supported(torch.float32, 16, 4, 32)
    assert not _lib.supported(torch.bfloat16, 64, 2, 96)     # dv must be 2*hs
    assert not _lib.supported(torch.bfloat16, 48, 2, 96)     # head size not built (the Python layer pads it)
    # branch counts without an N-branch plan run as branch groups (csrc/capi.hip)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for hs in (16, 32, 64, 96, 128):
            for n in range(1, 9):
                assert _lib.supported(dt, hs, n, 2 * hs), (dt, hs, n)
    assert not _lib.supported(torch.bfloat16, 64, 0, 128)


def test_padded_head_sizes_without_gpu():
    """ops.padded_head: head sizes without a plan run in the next built one (diff: dv = 2 hs;
    control: N = 1, dv = hs), up to 128."""
    from differential_transformer_replication_amd import ops
    assert ops.padded_head(torch.bfloat16, 64, 2, 128) == 64
    assert ops.padded_head(torch.bfloat16, 48, 2, 96) == 64
    assert ops.padded_head(torch.float32, 8, 5, 16) == 16
    assert ops.padded_head(torch.bfloat16, 100, 3, 200) == 128
    assert ops.padded_head(torch.bfloat16, 80, 1, 80) == 96
    assert ops.padded_head(torch.bfloat16, 16, 1, 16) == 32
    assert ops.padded_head(torch.bfloat16, 136, 2, 272) == 256      # 129-256: the 16-bit head-size-256 plans
    assert ops.padded_head(torch.float16, 256, 3, 512) == 256
    assert ops.padded_head(torch.float32, 136, 2, 272) is None          # fp32 diff plans stop at 128
    assert ops.padded_head(torch.float32, 200, 1, 200) == 256           # the control's dv = hs plan
    assert ops.padded_head(torch.bfloat16, 264, 2, 528) is None
    assert ops.padded_head(torch.bfloat16, 64, 2, 64) is None        # dv = hs only for N = 1


def test_invalid_args_rejected_without_gpu():
    lib = _lib.load()
    a = _lib.AttnFwdArgs()
    a.dtype, a.B, a.T, a.H, a.n_terms, a.head_size, a.dv = 0, 1, 8, 1, 2, 64, 128
    a.dropout_p = 1.0
    assert lib.dta_attn_fwd(a, None) == -4            # dropout p outside [0, 1) refused
    a.dropout_p = 0.5
    assert lib.dta_attn_fwd(a, None) == -1            # null pointers refused (p = 0.5 itself is fine)
    a.dropout_p = 0.0
    a.head_size, a.dv = 48, 96
    assert lib.dta_attn_fwd(a, None) == -2
    assert lib.dta_attn_fwd(None, None) == -1
    # branch-group query: default caps, an explicit cap, and a negative cap (invalid, as in dta_attn_bwd)
    assert lib.dta_attn_bwd_dkdv_groups(_lib.DTA_BF16, 64, 3, 128, 0) == 2
    assert lib.dta_attn_bwd_dkdv_groups(_lib.DTA_BF16, 64, 3, 128, 4) == 1
    assert lib.dta_attn_bwd_dkdv_groups(_lib.DTA_BF16, 64, 3, 128, -1) == 0


def test_decode_misaligned_views_rejected_without_gpu():
    """dta_attn_decode checks alignment of all four operands (16-byte vector
    accesses); a misaligned V or O view is refused before anything launches."""
    lib = _lib.load()
    base = 0x10000                                      # fake, 16-byte aligned device addresses
    a = _lib.DecodeArgs()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = 0, 1, 2, 2, 64, 128
    a.length, a.t_cap, a.scale = 4, 8, 0.125
    ok = lambda p, st: _lib.DtaTensor(p, 8 * st, st, 128, 64)
    a.q, a.k_cache = ok(base, 512), ok(base + 4096, 512)
    a.coef, a.workspace = base + 8192, base + 8192 + 64
    a.v_cache = _lib.DtaTensor(base + 2, 8 * 256, 256, 128, 0)         # base off by one element
    a.o = ok(base, 256)
    assert lib.dta_attn_decode(a, None) == -1
    a.v_cache = _lib.DtaTensor(base, 8 * 257, 257, 128, 0)             # row stride not a 16-byte multiple
    assert lib.dta_attn_decode(a, None) == -1
    a.v_cache = _lib.DtaTensor(base, 8 * 256, 256, 128, 0)
    a.o = _lib.DtaTensor(base + 6, 256, 256, 128, 0)                  # misaligned output
    assert lib.dta_attn_decode(a, None) == -1
    a.o = _lib.DtaTensor(None, 256, 256, 128, 0)
    assert lib.dta_attn_decode(a, None) == -1


def _cases(golden, prefix):
    return sorted({f.split("/")[0] for f in golden.files if f.startswith(prefix)})


def _build(case, g: Golden):
    meta = [int(v) for v in g["meta"]]
    if case.startswith("diffhead"):
        hs, Cm, T, blk, layer = meta
        return D.DiffHead(hs, Cm, 0.0, blk)
    if case.startswith("mhdiff"):
        H, hs, Cm, T, blk, layer = meta
        return D.MultiHeadDiffAttention(H, hs, Cm, 0.0, blk)
    if case.startswith("althead"):
        N, hs, Cm, T, blk, layer = meta
        return ND.AlternatingDiffHead(hs, Cm, 0.0, blk, N)
    if case.startswith("mhalt"):
        N, H, hs, Cm, T, blk, layer = meta
        return ND.MultiHeadAlternatingDiffAttention(H, hs, Cm, 0.0, blk, N)
    if case == "ctrlmha":
        H, hs, Cm, T, blk = meta
        return C.MultiHeadAttention(H, hs, Cm, 0.0, blk)
    raise KeyError(case)


@pytest.mark.parametrize("prefix", ["diffhead", "mhdiff", "althead", "mhalt", "ctrlmha"])
def test_state_dict_keys_and_load(golden, prefix):
    for case in _cases(golden, prefix):
        g = Golden(golden, case)
        m = _build(case, g)
        sd = m.state_dict()
        ours = {k for k in sd if not k.endswith("tril")}
        assert ours == set(g.state_dict().keys()), case
        trils = [k for k in sd if k.endswith("tril")]
        assert len(trils) == max(1, len(getattr(m, "heads", [0])))
        ref_sd = dict(g.state_dict(torch.float32))
        for k in trils:                                   # a reference checkpoint carries tril
            ref_sd[k] = sd[k]
        m.load_state_dict(ref_sd, strict=True)
        for k, v in g.state_dict(torch.float32).items():
            if torch.is_complex(v):
                assert torch.equal(m.state_dict()[k], v), k
            else:
                assert torch.equal(m.state_dict()[k].float(), v.float()), k


def test_model_state_dict_keys(golden):
    for case, ctor in [("modeldiff", lambda: D.DiffTransformer(97, 64, 2, 2, 24, 0.0)),
                       ("modelalt", lambda: ND.AlternatingDiffTransformer(97, 64, 2, 2, 24, 0.0, n_terms=3)),
                       ("modelctrl", lambda: C.StandardTransformer(97, 64, 4, 2, 24, 0.0))]:
        g = Golden(golden, case)
        m = ctor()
        ours = {k for k in m.state_dict() if not k.endswith("tril")}
        assert ours == set(g.state_dict().keys()), case
        m.load_state_dict(g.state_dict(torch.float32), strict=True)


@pytest.mark.parametrize("key", ["alt3", "diff"])
def test_seeded_init_matches_reference_diff_models(key):
    """The bf16 curve fixtures' models (tests/golden/make_curve_golden_bf16.py): same seed ->
    the same initial state as the reference's, every floating state_dict entry by (sum, sum of
    squares) in sorted key order, so the GPU replay starts where the reference did."""
    z = np.load(os.path.join(GOLDEN, "golden_loss_curve_diffmodels.npz"))
    torch.manual_seed(1337)
    m = (ND.AlternatingDiffTransformer(12000, 384, 3, 4, 256, 0.0, n_terms=3) if key == "alt3"
         else D.DiffTransformer(12000, 512, 4, 4, 256, 0.0))
    sd = {k: v for k, v in m.state_dict().items() if v.is_floating_point()}
    assert sorted(sd) == list(z[key + "/init_keys"])
    got = np.array([[float(sd[k].double().sum()), float((sd[k].double() ** 2).sum())] for k in sorted(sd)])
    np.testing.assert_allclose(got, z[key + "/init_sums"], rtol=1e-12, atol=1e-9)   # summation order


def test_seeded_init_matches_reference(golden_curve):
    """Same seed -> the same initial weights as the reference cfg1 model, every parameter by its
    float64 (sum, sum of squares).  The fixture's sums and these are float64 reductions whose
    order follows the host's thread count and vector width, so each may be off its exact value
    by a few rounding steps of the summed magnitudes (seen: 1 ulp on a 16-thread host, 2 of 414
    sums).  The bar is 64 eps of sum|x| (of sum x^2): above twice a pairwise reduction's
    log2(n) eps bound for the largest parameter (n = 4.6M, 22 eps), below what one float32
    ulp of a typical weight changes."""
    torch.manual_seed(1337)
    m = D.DiffTransformer(12000, 384, 6, 6, 256, 0.0)
    ps = [p.detach().double() for p in m.parameters()]
    sums = np.array([float(p.sum()) for p in ps])
    sq = np.array([float(p.pow(2).sum()) for p in ps])
    assert sums.shape == golden_curve["curve/param_sum"].shape
    eps = np.finfo(np.float64).eps
    tol = 64 * eps * np.array([float(p.abs().sum()) for p in ps])
    assert np.all(np.abs(sums - golden_curve["curve/param_sum"]) <= tol)
    assert np.all(np.abs(sq - golden_curve["curve/param_sq"]) <= 64 * eps * sq)


def test_control_cpu_matches_golden(golden):
    """control.py is carried as PyTorch (not the hot path) and runs on CPU too."""
    g = Golden(golden, "ctrlmha")
    m = _build("ctrlmha", g).double()
    m.load_state_dict(g.state_dict(torch.float64), strict=True)
    x = torch.from_numpy(g["in0"]).double().requires_grad_(True)
    out = m(x)
    assert rel_err(out, g["out"]) < 1e-6
    (out * torch.from_numpy(g["gout"]).double()).sum().backward()
    assert rel_err(x.grad, g["grad_in0"]) < 1e-6


def test_hot_path_refuses_cpu():
    m = D.MultiHeadDiffAttention(2, 16, 64, 0.0, 32)
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.randn(1, 8, 64), 1)
    with pytest.raises(RuntimeError, match="HIP"):
        ND.MultiHeadAlternatingDiffAttention(2, 16, 64, 0.0, 32, 3)(torch.randn(1, 8, 64), 1)


def test_reference_errors_preserved():
    m = D.MultiHeadDiffAttention(2, 16, 64, 0.0, 8)
    with pytest.raises(RuntimeError):
        m(torch.randn(1, 9, 64), 1)                    # T > block_size
    with pytest.raises(RuntimeError):
        ND.AlternatingDiffHead(16, 32, 0.0, 8, 0)(torch.randn(1, 4, 32), 1)   # n_terms = 0
    h = D.MultiHeadDiffAttention(2, 16, 64, 0.1, 8).train()
    h.heads[1].dropout.p = 0.2                         # per-head p that differ: refused, not ignored
    with pytest.raises(NotImplementedError):
        h(torch.randn(1, 4, 64), 1)


def test_lambda_side_effects_and_coefficients():
    torch.manual_seed(0)
    m = D.MultiHeadDiffAttention(3, 8, 48, 0.0, 16)
    for p in m.parameters():
        if p.dim() == 1 and p.numel() == 8:
            p.data.normal_(0, 0.1)
    c = m.coefficients(3)
    for h, head in enumerate(m.heads):
        lam_ref = head.get_lambda(3)
        assert c[h, 0].item() == 1.0
        assert c[h, 1].item() == pytest.approx(-lam_ref.item(), rel=1e-6)
        assert head.lambda_init.item() == pytest.approx(0.8 - 0.6 * np.exp(-0.6), rel=1e-6)
    assert m.lambda_init.item() == pytest.approx(0.8)
    na = ND.MultiHeadAlternatingDiffAttention(2, 8, 32, 0.0, 16, 3)
    for p in na.parameters():
        if p.dim() == 1 and p.numel() == 8:
            p.data.normal_(0, 0.1)
    c = na.coefficients(2)
    for h, head in enumerate(na.heads):
        lam = head.get_lambda(2)
        assert torch.allclose(c[h], lam * torch.tensor([1.0, -1.0, 1.0]), rtol=1e-6)


def test_control_model_cpu_matches_golden(golden):
    """StandardTransformer end to end (logits returned as (B*T, V) with targets,
    like the reference), loss and every parameter gradient."""
    g = Golden(golden, "modelctrl")
    m = C.StandardTransformer(97, 64, 4, 2, 24, 0.0).double()
    m.load_state_dict(g.state_dict(torch.float64), strict=True)
    idx = torch.from_numpy(g["idx"])
    logits, loss = m(idx, torch.from_numpy(g["tgt"]))
    assert tuple(logits.shape) == tuple(g["logits"].shape)
    assert rel_err(logits, g["logits"]) < 1e-6
    loss.backward()
    for k, p in m.named_parameters():
        assert rel_err(p.grad, g[f"grad::{k}"]) < 1e-5, k


def test_swiglu_args_rejected_without_gpu():
    lib = _lib.load()
    a = _lib.SwigluArgs()
    a.dtype, a.rows, a.n = 0, 4, 12                     # n not a multiple of 8
    assert lib.dta_swiglu_fwd(a, None) == -2
    a.n = 16
    assert lib.dta_swiglu_fwd(a, None) == -1            # null pointers
    assert lib.dta_swiglu_bwd(None, None) == -1


def test_ln_io_dtype_rules_without_gpu():
    """A 16-bit y / dy beside an fp32 x only (dta_ln_args.io_dtype)."""
    lib = _lib.load()
    a = _lib.LnArgs()
    a.dtype, a.rows, a.C, a.io_dtype = _lib.DTA_BF16, 4, 64, 1 + _lib.DTA_BF16
    assert lib.dta_ln_fwd(a, None) == -2
    a.dtype, a.io_dtype = _lib.DTA_F32, 1 + _lib.DTA_F32
    assert lib.dta_ln_fwd(a, None) == -2
    a.io_dtype = 1 + _lib.DTA_BF16
    assert lib.dta_ln_fwd(a, None) == -1            # valid combination, null pointers


def test_ln_bwd_partial_alignment_without_gpu():
    """dta_ln_args.partial holds 16-byte rows (the ordered reduce's vector loads): a
    misaligned workspace is rejected before any launch; dw / db sizes are unchanged."""
    lib = _lib.load()
    fake = 1 << 20                                   # never dereferenced: rejected first
    a = _lib.LnArgs()
    a.dtype, a.rows, a.C = _lib.DTA_BF16, 4, 64
    a.x, a.x_stride, a.w, a.mean, a.rstd = fake, 64, fake, fake, fake
    a.dy, a.dy_stride, a.dx, a.dx_stride, a.dw, a.db = fake, 64, fake, 64, fake, fake
    a.partial = fake + 4
    assert lib.dta_ln_bwd(a, None) == -1
    assert lib.dta_ln_bwd_workspace_bytes(4096, 2048) >= 2 * 2048 * 4 * 512
