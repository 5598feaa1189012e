"""dta_attn_fwd / dta_attn_bwd through the C ABI at tensor layouts other than the packed one.

include/diffattn.h gives every dta_tensor its own element strides; ``ops.diff_attention`` only
ever passes one family of them (the views of one packed (B, T, W) buffer, contiguous O / dO /
q_rot).  Here the same logical values are laid out in other ways -- head-major, row-padded,
branch-outer, mixed, broadcast K / V -- and each call is made directly through ``_lib`` with
hand-built ``dta_tensor`` structs, in the stages and with the workspaces of
``ops._DiffAttention``.  Per (case, layout):

a. every result (O, Obr, LSE, dQ, dK, dV, d(coef), the rotated rows) is bitwise what the packed
   layout gives for the same values: a layout changes addresses, not arithmetic.  Layouts the
   LDS-DMA descriptors cannot serve (csrc/layout_checks.h: a branch outside its row's stride, a
   row extent of 2^31 bytes) run the same kernels with the tiles staged by address and are held
   to the same equality, with one exception that ``_dq_reseeded`` states: dQ of the bf16 plans
   without dropout, whose descriptor instantiation alone seeds its accumulators with the row
   constants (another rounding order), is held to (b) only on those layouts;
b. every result is within test_gpu_parity's tolerance of the fp64 oracle (``_oracle_core``; the
   mask restatement of test_gpu_dropout for the dropout case and, with all-ones masks, for the
   control model's dv = head_size, which ``_oracle_core`` does not take);
c. all storage is carved from 0xFF-filled buffers (``_poison.Arena``): every guard byte and every
   hole byte (pad columns, unused regions) is still 0xFF afterwards and every output element is
   finite, so a store that ignores a stride is an assertion failure in memory the test owns.
"""
import collections
import functools
import math

import pytest
import torch

from _poison import Arena
from conftest import rel_err
from oracle import diffattn_oracle as orc
from test_gpu_dropout import _oracle_dropped, drop_masks
from test_gpu_parity import DEV, TOL, _oracle_core, _rope64

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SEED = 0x1234_5678_9ABC

Case = collections.namedtuple("Case", "dtype N hs dv rope p caps Ts layouts")
ALL = ("L0", "L1", "L2", "L3", "L4", "L5", "L6")


def _case(dtype, N, hs, dv=None, rope=False, p=0.0, caps=(0, 0), Ts=(70, 200), layouts=ALL):
    return Case(dtype, N, hs, 2 * hs if dv is None else dv, rope, p, caps, Ts, layouts)


# T = 70 and 200: a ragged last tile and more than one key tile in every plan; H = 2, B = 2
CASES = [
    _case(BF16, 2, 64), _case(F16, 2, 64),              # the paired plan
    _case(BF16, 3, 64, rope=True),                      # q_rot's layout, dK/dV in branch groups (dv_f32)
    _case(BF16, 2, 128),
    _case(BF16, 1, 64, dv=64),                          # the control plan
    _case(BF16, 2, 16),                                 # no LDS-DMA
    _case(F32, 2, 64), _case(F32, 3, 32, rope=True),
    _case(BF16, 2, 256, Ts=(70,)),                      # single-branch groups in the backward
    _case(BF16, 2, 64, p=0.1),                          # the separately compiled *_drop kernels
    _case(BF16, 4, 32, caps=(4, 4), layouts=("L0", "L1", "L4")),      # the native 4-branch backward
]

# ---------------------------------------------------------------------------- layouts ---
QLIKE = ("q", "k", "dq", "dk", "qrot", "krot")          # [b][t][h][i][d]
VLIKE = ("v", "o", "do", "dv")                          # [b][t][h][e]
LOGICAL = {**{n: "bthid" for n in QLIKE}, **{n: "bthe" for n in VLIKE}, "obr": "ibthe"}
# what ops passes: three packed buffers' views, the rest contiguous
PACKED = {"q": ("qkv", 0), "k": ("qkv", 1), "v": ("qkv", 2), "dq": ("dqkv", 0), "dk": ("dqkv", 1), "dv": ("dqkv", 2),
          "qrot": ("rot", 0), "krot": ("rot", 1)}


def own(order, pad=0, bcast=False):
    """A tensor in a buffer of its own: dimensions outermost first, ``pad`` elements added to
    the row (t) stride, ``bcast``: one batch row stored, sb = 0 (inputs only)."""
    return (order, pad, bcast)


LAYOUTS = {
    # L0 packed: exactly what ops passes, the baseline
    "L0": {},
    # L1 head-major, the (B, H, T, D) convention: st < sh, and (N - 1) si + hs = st exactly
    "L1": {**{n: own("bhtid") for n in QLIKE}, **{n: own("bhte") for n in VLIKE}, "obr": own("ibhte")},
    # L2 separate row-padded buffers: st = H N hs + 8 (H dv + 8); the pad columns are holes
    "L2": {**{n: own("bthid", 8) for n in QLIKE}, **{n: own("bthe", 8) for n in VLIKE}, "obr": own("ibthe", 8)},
    # L3 branch-interleaved-outer: si = H hs > sh
    "L3": {n: own("btihd") for n in QLIKE},
    # L4 branch-outer: si = T H hs = T st, every branch but the first outside its row's stride
    "L4": {n: own("bithd") for n in QLIKE},
    # L5 mixed: inputs L0, gradients L1, O L2, q_rot L3 -- no kernel borrows another tensor's strides
    "L5": {"dq": own("bhtid"), "dk": own("bhtid"), "dv": own("bhte"), "o": own("bthe", 8), "qrot": own("btihd"),
           "krot": own("bthid")},
    # L6 one K / V for both batch rows: k.sb = v.sb = 0 (the values are those rows expanded)
    "L6": {"k": own("bthid", 0, True), "v": own("bthe", 0, True)},
}


def _sizes(case, B, T, H):
    return {"b": B, "t": T, "h": H, "i": case.N, "d": case.hs, "e": case.dv}


def _place(case, B, T, H, layout, dev):
    """name -> view (logical dimension order) of every dta_tensor of a call, and the arenas."""
    sz = _sizes(case, B, T, H)
    nq, arenas, groups, views = H * case.N * case.hs, [], {}, {}
    width = {"qkv": 2 * nq + H * case.dv, "dqkv": 2 * nq + H * case.dv, "rot": 2 * nq}
    names = list(QLIKE if case.rope else QLIKE[:4]) + list(VLIKE) + ["obr"]
    for name in names:
        dtype = F32 if name == "obr" else case.dtype
        logical = LOGICAL[name]
        if name in layout:
            order, pad, bcast = layout[name]
            stride, run = {}, 1
            for n in reversed(order):
                if n == "b" and bcast:
                    stride[n] = 0
                    continue
                stride[n] = run + (pad if n == "t" else 0)
                run = stride[n] * sz[n]
            arena = Arena(run * dtype.itemsize, dev, name)
            arenas.append(arena)
            views[name] = arena.view(dtype, [sz[n] for n in logical], [stride[n] for n in logical])
        elif name in PACKED:
            group, part = PACKED[name]
            W = width[group]
            if group not in groups:
                groups[group] = Arena(B * T * W * dtype.itemsize, dev, group)
                arenas.append(groups[group])
            inner = (case.dv, 1) if name in VLIKE else (case.N * case.hs, case.hs, 1)
            views[name] = groups[group].view(dtype, [sz[n] for n in logical], (T * W, W) + inner, part * nq)
        else:                                                   # O, dO, Obr: contiguous
            shape = [sz[n] for n in logical]
            arena = Arena(math.prod(shape) * dtype.itemsize, dev, name)
            arenas.append(arena)
            views[name] = arena.view(dtype, shape, torch.empty(shape, device="meta").stride())
    return views, arenas


def _fill(view, vals):
    """Write an input through its view (a broadcast one through its single batch row)."""
    if view.stride(0) == 0 and view.shape[0] > 1:
        assert all(torch.equal(vals[:1], vals[b:b + 1]) for b in range(1, vals.shape[0]))
        view[:1].copy_(vals[:1])
    else:
        view.copy_(vals)


class Results(dict):
    """name -> result of one call; ``inexact``: the results held to (b) only, not to (a)."""
    inexact = ()


def _dq_reseeded(case, T, k, v):
    """Whether the dQ kernel of this call rounds differently from the packed layout's.

    One code path does depend on the layout, legitimately: the bf16 dQ kernel without dropout
    starts its score and dP accumulators at the row constants (-LSE_i, -delta_0) through an extra
    MFMA k-step, and (attn_kernels.h, attn_dq_kernel's SEED) only in the instantiation that stages
    K / V through the LDS-DMA descriptors, which the 16-bit plans with head size >= 32 select when
    csrc/layout_checks.h admits the K / V strides of the launch's branch group.  Elsewhere the
    constants are added to the finished fp32 sums: the same mathematics, another rounding order,
    in dQ alone (delta, d(coef) and the key-major kernel do not change).  dQ is then held to the
    fp64 tolerance only."""
    if case.dtype != BF16 or case.p or case.hs < 32:
        return False
    # branches per dQ launch: group_max_dq and its defaults (include/diffattn.h; head size 256: 1)
    cap = case.caps[0] or (1 if case.hs >= 192 else 2 if case.hs >= 128 or (case.hs == 64 and case.N >= 4) else 4)
    g = min(case.N, cap)
    if case.hs >= 128 and g >= 3:
        return False
    kst, ksi, vst = k.stride(1), k.stride(3), v.stride(1)
    return (g - 1) * ksi + case.hs > kst or case.dv > vst or T * max(kst, vst) * 2 >= 2 ** 31


def _run(case, vals, layout, given=None):
    """One forward and backward through the C ABI at ``layout``; ``given``: views the caller laid
    out itself, inputs (which it also filled) or outputs (tests/test_gpu_far_addresses.py).
    Checks (c) and returns the results, contiguous."""
    from differential_transformer_replication_amd import _lib
    lib = _lib.load()
    dev = vals["q"].device
    B, T, H = vals["q"].shape[:3]
    N, hs, dv, dt = case.N, case.hs, case.dv, _lib.dtype_code(case.dtype)
    assert lib.dta_supported(dt, hs, N, dv)
    views, arenas = _place(case, B, T, H, layout, dev)
    views.update(given or {})
    for name in ("q", "k", "v", "do"):
        if not (given and name in given):
            _fill(views[name], vals[name])

    def work(name, *shape):                                     # fp32 outputs and workspaces, contiguous
        arena = Arena(math.prod(shape) * 4, dev, name)
        arenas.append(arena)
        return arena.view(F32, shape, torch.empty(shape, device="meta").stride())

    t5 = _lib.tensor5
    obr = views["obr"]
    obr_t = _lib.DtaTensor(obr.data_ptr(), *obr.stride()[1:4], obr.stride(0))
    lse = work("lse", N, B, H, T)
    coef = vals["coef"]
    stream = _lib.stream_handle(dev)
    scale = 1.0 / math.sqrt(hs)
    freqs, k, rope_args = vals["freqs"], views["k"], (None, _lib.DtaTensor())
    if case.rope:
        ra = _lib.RopeArgs(dt, B, T, H, N, hs, 0, 0, t5(k), t5(views["krot"]), freqs.data_ptr())
        _lib.check(lib.dta_rope(ra, stream))
        k = views["krot"]
        rope_args = (freqs.data_ptr(), t5(views["qrot"]))
    fa = _lib.AttnFwdArgs(dt, B, T, H, N, hs, dv, scale, case.p, t5(views["q"]), t5(k), t5(views["v"]), t5(views["o"]),
                          obr_t, lse.data_ptr(), coef.data_ptr(), SEED, *rope_args, _lib.DTA_F32)
    _lib.check(lib.dta_attn_fwd(fa, stream))

    q = views["qrot"] if case.rope else views["q"]
    dcoef, delta = work("dcoef", H, N), work("delta", N, B, H, T)
    dcp = work("dcp", lib.dta_attn_bwd_dcoef_partial_bytes(B, T, H, N) // 4)
    dv32 = lsec = None
    if dt != _lib.DTA_F32 and lib.dta_attn_bwd_dkdv_groups(dt, hs, N, dv, case.caps[1]) > 1:
        dv32 = work("dv32", B, T, H, dv)
    if dt != _lib.DTA_F32 and case.p == 0.0:
        lsec = work("lsec", N, B, H, T)
    ba = _lib.AttnBwdArgs(dt, B, T, H, N, hs, dv, scale, case.p, t5(q), t5(k), t5(views["v"]), obr_t,
                          lse.data_ptr(), coef.data_ptr(), t5(views["do"]),
                          t5(views["dq"]), t5(views["dk"]), t5(views["dv"]),
                          dcoef.data_ptr(), delta.data_ptr(), None, _lib.BWD_DQ,
                          freqs.data_ptr() if case.rope else None, dcp.data_ptr(), SEED, _lib.DTA_F32, *case.caps,
                          dv32.data_ptr() if dv32 is not None else None,
                          lsec.data_ptr() if lsec is not None else None)
    _lib.check(lib.dta_attn_bwd(ba, stream))
    ba.stages = _lib.BWD_DKDV
    _lib.check(lib.dta_attn_bwd(ba, stream))
    torch.cuda.synchronize()

    for arena in arenas:                                        # (c): guards and holes, then finiteness
        arena.check()
    out = Results({n: views[n].contiguous() for n in ("o", "obr", "dq", "dk", "dv") + (("qrot", "krot") if case.rope else ())})
    out.update(lse=lse.clone(), dcoef=dcoef.clone())
    out.inexact = ("dq",) if _dq_reseeded(case, T, k, views["v"]) else ()
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{name}: unwritten or poison-derived elements"
    return out


# -------------------------------------------------------------------- values, reference ---
def _values(case, T, B=2, H=2, shared_kv=False):
    """The logical values of a case: one packed (B, T, W) tensor, coef and dO, as test_gpu_parity
    draws them; ``shared_kv``: K and V of every batch row are those of row 0."""
    from differential_transformer_replication_amd import ops
    g = torch.Generator().manual_seed(1000 * H + 100 * case.N + case.hs + T)
    qkv = torch.randn(B, T, ops.packed_width(H, case.N, case.hs, case.dv), generator=g).to(case.dtype)
    coef = torch.randn(H, case.N, generator=g) * 0.5
    coef[:, 0] = 1.0
    do = torch.randn(B, T, H, case.dv, generator=g).to(case.dtype)
    if shared_kv:
        qkv[1:, :, H * case.N * case.hs:] = qkv[:1, :, H * case.N * case.hs:]
    q, k, v = ops.split_packed(qkv.to(DEV), H, case.N, case.hs, case.dv)
    return _with_tables(case, T, {"q": q, "k": k, "v": v, "do": do.to(DEV), "coef": coef.to(DEV)})


def _with_tables(case, T, vals):
    vals["freqs_c"] = orc.precompute_freqs_cis(case.hs, max(T, 8)) if case.rope else None
    vals["freqs"] = torch.view_as_real(vals["freqs_c"][:T]).contiguous().to(DEV) if case.rope else None
    return vals


def _reference(case, vals):
    """fp64 on the CPU: O and the gradients by the project's oracles, O_i and LSE_i restated."""
    B, T, H = vals["q"].shape[:3]
    N, hs, dv = case.N, case.hs, case.dv
    x64 = torch.cat([vals[n].flatten(2) for n in ("q", "k", "v")], dim=-1).double().cpu().requires_grad_(True)
    c64 = vals["coef"].double().cpu().requires_grad_(True)
    fc = vals["freqs_c"]
    masks = drop_masks(SEED, case.p, B, H, N, T) if case.p else torch.ones(1, H, N, 1, 1, dtype=torch.float64)
    if case.p or dv != 2 * hs:
        o = _oracle_dropped(x64, c64, H, N, hs, dv, masks, fc)
    else:
        o = _oracle_core(x64, c64, H, N, hs, fc)
    o.backward(vals["do"].flatten(2).double().cpu())
    nq = H * N * hs
    ref = {"o": o.detach().view(B, T, H, dv), "dq": x64.grad[..., :nq].view(B, T, H, N, hs),
           "dk": x64.grad[..., nq:2 * nq].view(B, T, H, N, hs), "dv": x64.grad[..., 2 * nq:].view(B, T, H, dv),
           "dcoef": c64.grad}
    q, k, v = (vals[n].double().cpu() for n in ("q", "k", "v"))
    obr, lse = torch.empty(N, B, T, H, dv, dtype=torch.float64), torch.empty(N, B, H, T, dtype=torch.float64)
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for h in range(H):
        for i in range(N):
            qi, ki = q[:, :, h, i], k[:, :, h, i]
            if fc is not None:
                qi, ki = _rope64(qi, fc), _rope64(ki, fc)
            s = (qi @ ki.transpose(-2, -1) / math.sqrt(hs)).masked_fill(~causal, float("-inf"))
            lse[i, :, h] = -torch.logsumexp(s, dim=-1) / math.log(2.0)          # the header's negated log2-sum-exp
            obr[i, :, :, h] = (orc.causal_softmax(qi, ki, 1.0 / math.sqrt(hs)) * masks[:, h, i]) @ v[:, :, h]
    ref.update(obr=obr, lse=lse)
    return ref


@functools.lru_cache(maxsize=None)
def _baseline(case, T, shared_kv):
    """(values, fp64 reference, the packed layout's results) of a case, computed once."""
    vals = _values(case, T, shared_kv=shared_kv)
    return vals, _reference(case, vals), _run(case, vals, LAYOUTS["L0"])


def _assert_bitwise(out, base, but=()):
    differ = [name for name in base if not torch.equal(out[name].view(torch.uint8), base[name].view(torch.uint8))]
    assert differ == [n for n in differ if n in but], f"{differ} differ from the packed layout's"       # (a)


def _assert_parity(case, out, ref):
    for name in ref:                                            # (b)
        err = rel_err(out[name].float().cpu(), ref[name])
        assert err < TOL[case.dtype], f"{name}: {err:.3g}"


def _id(case):
    return (f"{str(case.dtype)[6:]}-N{case.N}-hs{case.hs}" + ("-ctrl" if case.dv == case.hs else "")
            + ("-rope" if case.rope else "") + ("-drop" if case.p else "") + ("-native4" if case.caps[0] else ""))


PARAMS = [pytest.param(c, T, L, id=f"{_id(c)}-T{T}-{L}") for c in CASES for T in c.Ts for L in c.layouts]


@pytest.mark.parametrize("case,T,layout", PARAMS)
def test_layout(case, T, layout):
    vals, ref, base = _baseline(case, T, layout == "L6")
    out = base
    if layout != "L0":
        out = _run(case, vals, LAYOUTS[layout])
        _assert_bitwise(out, base, out.inexact)
    _assert_parity(case, out, ref)


# ------------------------------------------------------- the descriptor condition's edges ---
@pytest.mark.parametrize("past", [0, 8], ids=["equality", "16-bytes-past"])
def test_row_stride_boundary(past):
    """Each side of (N - 1) si + hs <= st (and dv <= st for V / dO), the condition of the LDS-DMA
    descriptors (csrc/layout_checks.h).  Q / K: st = N hs with si = hs (equality) or hs + 8
    elements, so the last 16 bytes of a row's second branch are the first 16 of the next row's
    first; V / dO: st = dv or dv - 8.  Read-only views may overlap, so the storage is drawn
    first and the logical values are read back through the views.  A descriptor built for the
    row stride would return zeros for the last row's overhang."""
    case, B, T, H = _case(BF16, 2, 64), 2, 70, 2
    N, hs, dv = case.N, case.hs, case.dv
    g = torch.Generator().manual_seed(90 + past)
    given, arenas = {}, []
    for name in ("q", "k", "v", "do"):
        if name in QLIKE:
            st = N * hs
            shape, strides = (B, T, H, N, hs), (H * (T * st + 8), st, T * st + 8, hs + past, 1)
        else:
            st = dv - past
            shape, strides = (B, T, H, dv), (H * T * dv, st, T * dv, 1)
        n = B * strides[0]
        arena = Arena(n * 2, DEV, name)
        arena.view(BF16, (n,), (1,)).copy_(torch.randn(n, generator=g))
        given[name] = arena.view(BF16, shape, strides)
        arenas.append(arena)
    if past:
        assert given["k"][0, 0, 0, 1, hs - 8:].data_ptr() == given["k"][0, 1, 0, 0].data_ptr()
        assert given["v"][0, 0, 0, dv - 8:].data_ptr() == given["v"][0, 1, 0].data_ptr()
    vals = {name: v.contiguous() for name, v in given.items()}
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    vals = _with_tables(case, T, {**vals, "coef": coef.to(DEV)})
    base = _run(case, vals, LAYOUTS["L0"])
    out = _run(case, vals, LAYOUTS["L0"], given=given)
    for arena in arenas:
        arena.check()
    assert out.inexact == (("dq",) if past else ()) and not base.inexact
    _assert_bitwise(out, base, out.inexact)
    _assert_parity(case, out, _reference(case, vals))


def test_row_extent_past_32_bits():
    """K rows 2^25 elements (64 MiB) apart: T st es = 70 * 2^26 bytes is past the descriptors' 32-bit
    record count, so the launch has to stage K by 64-bit addresses; O and the gradients are bitwise
    the packed layout's.  The 4.6 GB allocation is real and the test's own (only the 70 rows are
    ever written), so whatever a library reads of it is memory this test owns."""
    case, B, T, H = _case(BF16, 2, 64), 1, 70, 1
    vals = _values(case, T, B=B, H=H)
    base = _run(case, vals, LAYOUTS["L0"])
    st = 2 ** 25
    big = k = None
    try:
        big = torch.empty((T - 1) * st + case.N * case.hs, dtype=BF16, device=DEV)
        k = big.as_strided((B, T, H, case.N, case.hs), (T * st, st, case.N * case.hs, case.hs, 1))
        k.copy_(vals["k"])
        out = _run(case, vals, LAYOUTS["L0"], given={"k": k})
    finally:
        del big, k
        torch.cuda.empty_cache()
    assert out.inexact == ("dq",) and not base.inexact
    _assert_bitwise(out, base, out.inexact)
    _assert_parity(case, out, _reference(case, vals))
