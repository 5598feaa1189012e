"""Every strided operand far from its base pointer: beyond 2 GiB, 4 GiB and 2^31 fp32 elements.

The rest of the suite keeps every operand within a few MiB of the pointer it passes, so an
``int`` or ``uint32_t`` temporary in a kernel's ``index * stride`` would pass all of it.  Each
case here (the list is ``_far.cases()``, which tests/test_far_cpu.py checks in integers) gives
one dimension of one operand a stride -- or, for a page pool, a real size -- that puts part of
it at far-2 / far-4 / far-8 (tests/_far.py), and then, per case:

1. runs the op on the compact layout;
2. runs it on the far layout with the same values;
3. asserts the results bitwise equal: a layout changes addresses, not arithmetic.  The one
   exception is test_gpu_abi_layouts's ``_dq_reseeded``: a far *row* stride of K or V takes the
   bf16 dQ kernel off the LDS-DMA descriptors (T st es >= 2^31), which reseeds its accumulators;
4. asserts the far result within the family's ``TOL[dtype]`` of the fp64 oracle its own tests
   use (``_oracle_core`` / ``_oracle_dropped`` for the training core, ``O.diff_core`` per
   sequence for the caches).

The far operand lives in a ``_far.FarBuffer``: 0xFF everywhere, holding every address a 32-bit
truncation of the offset would reach (up to 4 GiB below the base pointer), so a wrong address
reads NaN or is found by the after-check, which also holds every byte outside the operand's
elements to 0xFF.  Every output element must be finite.  At most 10 GiB are live in a test; the
only skip is too little free device memory.

The far-8 cases (fp32 k of the training core, fp32 K cache, LayerNorm's fp32 x) own every wrong
image but one: the sign-extended *element* offset lies 8 GiB below the base pointer, which with
the 8 GiB above it no buffer under the cap can hold (``Placement.out_of_reach``).
"""
import functools
import math

import pytest
import torch

import _far
import test_gpu_abi_layouts as ABI
import test_gpu_ragged as R
import test_gpu_rowwise_matrix as RM
import _rowwise as rw
from conftest import rel_err
from oracle import diffattn_oracle as O

from differential_transformer_replication_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPE = {2: BF16, 4: F32}


def _with_far(c, dtypes, body):
    """``body(*buffers)`` with the case's far buffer(s); they (and, ``body`` having returned,
    every view of them) are released whatever happened."""
    places = _far.placements(c)
    dtypes = dtypes if isinstance(dtypes, (tuple, list)) else (dtypes,)
    _far.skip_unless_free(_far.need(*[p.nbytes for p in places]))
    fbs = []
    try:
        for p, dtype in zip(places, dtypes):
            fbs.append(_far.FarBuffer(p, dtype, DEV))
        return body(*fbs)
    finally:
        for fb in fbs:
            fb.release()
        del fbs
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------ training core ---
TRAIN_CASES = {"bf16-N2": ABI._case(BF16, 2, 64), "bf16-N3-rope": ABI._case(BF16, 3, 64, rope=True),
               "f32-N2": ABI._case(F32, 2, 64), "bf16-N2-drop": ABI._case(BF16, 2, 64, p=0.1)}


@pytest.mark.parametrize("c", _far.cases("train"), ids=_far.case_id)
def test_training_core(c):
    """dta_attn_fwd / dta_attn_bwd through test_gpu_abi_layouts's ``_run`` with one operand on a
    far batch, head or row stride, the others as ``ops`` passes them.  A far batch or head
    stride leaves T st es small, so the descriptor path stays selected and its per-tile 64-bit
    base is what is tested; a far row stride takes the operand's tiles by 64-bit addresses.
    far-8 (fp32 k): the sign-extended element image, 8 GiB below, is the one address not owned."""
    case = TRAIN_CASES[c.key]
    es, N, hs, dv, rope, p = _far.TRAIN[c.key]
    assert (case.dtype.itemsize, case.N, case.hs, case.dv, case.rope, case.p) == (es, N, hs, dv, rope, p)
    vals, ref, base = ABI._baseline(case, _far.TRAIN_T, False)
    assert tuple(vals["q"].shape[:3]) == (_far.TRAIN_B, _far.TRAIN_T, _far.TRAIN_H)

    def body(fb):
        if c.operand in ("q", "k", "v", "do"):
            fb.view.copy_(vals[c.operand])
        out = ABI._run(case, vals, ABI.LAYOUTS["L0"], given={c.operand: fb.view})      # finiteness: inside
        fb.check()
        return out

    out = _with_far(c, F32 if c.operand == "obr" else case.dtype, body)
    # the staging mode changes only where the row stride of the dQ kernel's K / V is the far one
    switched = c.dim == "t" and c.operand in ("k", "v") and case.dtype == BF16 and not case.p
    assert out.inexact == (("dq",) if switched else ()) and not base.inexact
    ABI._assert_bitwise(out, base, out.inexact)
    ABI._assert_parity(case, out, ref)


# --------------------------------------------------------------------- contiguous cache ---
B, H, CAP, TQ, LENGTHS = _far.CACHE_B, _far.CACHE_H, _far.CACHE_CAP, _far.CACHE_TQ, _far.CACHE_LENGTHS
ROWS_TQ, ROWS_COUNTS = 5, (5, 5, 3)
# op -> (pos, counts) of its rows: a decode at length L is one row at position L - 1
STEPS = {"decode_ragged": (tuple(L - 1 for L in LENGTHS), (1,) * B),
         "decode": ((CAP - 1,) * B, (1,) * B),
         "extend_ragged": (tuple(L - TQ for L in LENGTHS), (TQ,) * B),
         "extend": ((CAP - TQ,) * B, (TQ,) * B),
         "decode_rows": (tuple(L - ROWS_TQ for L in LENGTHS), ROWS_COUNTS)}


# the paged entry points compute the contiguous ones' steps
PAGED_STEP = {"decode_paged": "decode_ragged", "decode_shared": "decode_ragged", "extend_ragged_paged": "extend_ragged",
              "decode_rows_paged": "decode_rows"}


@functools.lru_cache(maxsize=None)
def _cache_inputs(key):
    """q rows (B, TQ, H, N, hs), caches of CAP rows, coef.  Sequence 2's first 256 rows are
    sequence 0's (the prefix the shared-prefix decode reads once)."""
    N, hs, dv = _far.CACHE[key]
    g = torch.Generator().manual_seed(31 * N + hs + dv)
    q = torch.randn(B, TQ, H, N, hs, generator=g)
    k = torch.randn(B, CAP, H, N, hs, generator=g)
    v = torch.randn(B, CAP, H, dv, generator=g)
    k[2, :256], v[2, :256] = k[0, :256], v[0, :256]
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    return q, k, v, coef


@functools.lru_cache(maxsize=None)
def _cache_want(key, dtype, op):
    """fp64 oracle of one step on the values as ``dtype`` holds them, per sequence: the rows
    pos .. pos + count - 1 of ``O.diff_core`` over the first pos + count cache rows (as
    test_gpu_ragged's ``_dec_want`` / ``_ext_case``).  Computed once, shared read-only."""
    N, hs, dv = _far.CACHE[key]
    q, k, v, coef = _cache_inputs(key)
    q, k, v = (t.to(dtype).double() for t in (q, k, v))
    pos, counts = STEPS[op]
    want = torch.zeros(B, max(counts), H, dv, dtype=torch.float64)
    for b in range(B):
        n, L = counts[b], pos[b] + counts[b]
        for h in range(H):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs, dtype=torch.float64)
                rows[0, pos[b]:] = q[b, :n, h, i]
                qs.append(rows)
            o = O.diff_core(qs, [k[b:b + 1, :L, h, i] for i in range(N)], v[b:b + 1, :L, h], coef[h].double())
            want[b, :n, h] = o[0, pos[b]:]
    return want


def _cache_ops(key):
    N, hs, dv = _far.CACHE[key]
    return ("decode_ragged", "decode") + (("extend_ragged", "extend", "decode_rows") if hs % 16 == 0 else ())


def _cache_run(key, q, k, v, coef):
    """op -> (B, rows, H, dv) of every contiguous-cache entry point on these views."""
    N, hs, dv = _far.CACHE[key]
    i32 = R._i32
    out = {}
    for op in _cache_ops(key):
        pos, counts = STEPS[op]
        if op == "decode_ragged":
            o = ops.diff_attention_decode_ragged(q[:, 0], k, v, coef, i32(LENGTHS))
        elif op == "decode":
            o = ops.diff_attention_decode(q[:, 0], k, v, coef, CAP)
        elif op == "extend_ragged":
            o = ops.diff_attention_extend_ragged(q, k, v, coef, i32(pos))
        elif op == "extend":
            o = ops.diff_attention_extend(q, k, v, coef, pos[0])
        else:
            assert ops.decode_rows_supported(q.dtype, hs, N, dv, ROWS_TQ)
            o = ops.diff_attention_decode_rows(q[:, :ROWS_TQ], k, v, coef, i32(pos), i32(counts))
        out[op] = o.view(B, -1, H, dv)
    torch.cuda.synchronize()
    return out


def _check_steps(key, dtype, far, compact, tag):
    for op, got in far.items():
        assert torch.equal(got, compact[op]), (tag, op, "the far layout's result differs from the compact one's")
        assert bool(torch.isfinite(got).all()), (tag, op)
        step = PAGED_STEP.get(op, op)
        want, counts = _cache_want(key, dtype, step), STEPS[step][1]
        for b in range(B):
            err = rel_err(got[b, :counts[b]].float(), want[b, :counts[b]])
            print(f"{tag} {op} b={b}: rel_err {err:.3e}")
            assert err <= R.TOL[dtype], (tag, op, b, err)
            assert bool((got[b, counts[b]:] == 0).all()), (tag, op, b, "padding rows are zeros")


@functools.lru_cache(maxsize=None)
def _cache_compact(key, dtype):
    q, k, v, coef = _cache_inputs(key)
    dev = [t.to(DEV, dtype) for t in (q, k, v)] + [coef.to(DEV)]
    return dev, _cache_run(key, *dev)


def _cache_run_abi(key, q, k, v, coef, o):
    """``_cache_run`` through the C ABI with the caller's o (B, TQ, H, dv): ``ops`` allocates o
    itself, contiguous, so a far o is a layout ``ops`` cannot pass and the C ABI accepts.  The
    argument structs are built as ``ops._decode`` / ``_extend`` / ``_decode_rows`` build them; o is
    poisoned again before every op."""
    N, hs, dv = _far.CACHE[key]
    lib, t5, i32 = _lib.load(), _lib.tensor5, R._i32
    dt, scale, stream = _lib.dtype_code(q.dtype), 1.0 / math.sqrt(hs), _lib.stream_handle(q.device)
    coef = coef.float().contiguous()
    ws = torch.empty(max(lib.dta_attn_decode_workspace_bytes(B, H, N, hs, dv, CAP),
                         lib.dta_attn_decode_rows_workspace_bytes(B, H, N, hs, dv, CAP, ROWS_TQ)
                         if "decode_rows" in _cache_ops(key) else 0) // 4, device=DEV)
    keep, out = [], {}
    for op in _cache_ops(key):
        pos, counts = STEPS[op]
        rows = max(counts)
        ov = o[:, :rows]
        ov.view(torch.int16 if o.element_size() == 2 else torch.int32).fill_(-1)
        if op in ("decode_ragged", "decode"):
            head = (dt, B, H, N, hs, dv, CAP, CAP, scale, t5(q[:, :1]), t5(k), t5(v), t5(ov), coef.data_ptr(), ws.data_ptr())
            if op == "decode":
                rc = lib.dta_attn_decode(_lib.DecodeArgs(*head, None), stream)
            else:
                keep.append(i32(LENGTHS))
                rc = lib.dta_attn_decode_ragged(_lib.DecodeRaggedArgs(*head, keep[-1].data_ptr()), stream)
        elif op in ("extend_ragged", "extend"):
            head = (dt, B, H, N, hs, dv, TQ)
            mid = (CAP, scale, t5(q), t5(k), t5(v), t5(ov), coef.data_ptr())
            if op == "extend":
                rc = lib.dta_attn_extend(_lib.ExtendArgs(*head, pos[0], *mid), stream)
            else:
                keep.append(i32(pos))
                rc = lib.dta_attn_extend_ragged(_lib.ExtendRaggedArgs(*head, *mid, keep[-1].data_ptr(), None), stream)
        else:
            keep += [i32(pos), i32(counts)]
            head = (dt, B, H, N, hs, dv, ROWS_TQ, CAP, scale, t5(q[:, :ROWS_TQ]), t5(k), t5(v), t5(ov), coef.data_ptr(),
                    ws.data_ptr(), keep[-2].data_ptr(), keep[-1].data_ptr())
            rc = lib.dta_attn_decode_rows(_lib.DecodeRowsArgs(*head), stream)
        _lib.check(rc)
        torch.cuda.synchronize()
        out[op] = ov.contiguous()
    return out


@pytest.mark.parametrize("c", _far.cases("cache"), ids=_far.case_id)
def test_contiguous_cache(c):
    """diff_attention_decode / _decode_ragged / _decode_rows / _extend / _extend_ragged with the K
    cache, the V cache, q or o on a far batch stride (the last sequence, 600 rows, lies beyond)
    or a far row stride (the crossing lies inside every sequence that reaches it).  A far o goes
    through ``_lib`` (``_cache_run_abi``): ``ops`` allocates o itself.  far-8 (fp32 K): the
    sign-extended element image, 8 GiB below, is the one address not owned."""
    dtype = DTYPE[c.placement.es]
    (q, k, v, coef), compact = _cache_compact(c.key, dtype)

    def body(fb):
        if c.operand == "o":
            far = _cache_run_abi(c.key, q, k, v, coef, fb.view)
        else:
            fb.view.copy_({"q": q, "k": k, "v": v}[c.operand])
            far = _cache_run(c.key, **{**dict(q=q, k=k, v=v, coef=coef), c.operand: fb.view})
        fb.check()
        return far

    _check_steps(c.key, dtype, _with_far(c, dtype, body), compact, _far.case_id(c))


# -------------------------------------------------------------------------- paged cache ---
def _paged_table(P, ids):
    """(table (B, PAGED_CAP / P) int32 with -1 in the unused entries, page -> (b, first row))
    from page ids dealt in order: consecutive pages of a sequence fall in different bands, so
    every 256-key chunk's pages straddle the thresholds; sequence 2's first 256 rows are
    sequence 0's pages."""
    per, count = _far.paged_pages(P)
    assert len(ids) == count
    table = torch.full((B, _far.PAGED_CAP // P), -1, dtype=torch.int32)
    owner, rest = {}, list(ids)
    for b in range(B):
        for p in range(per[b]):
            if b == 2 and p < 256 // P:
                table[b, p] = table[0, p]
                continue
            table[b, p] = rest.pop(0)
            owner[int(table[b, p])] = (b, p * P)
    assert not rest
    return table.to(DEV), owner


def _paged_run(pool, table, q, coef, P):
    N, hs, dv = _far.CACHE["N2-hs64"]
    nq = H * N * hs
    k_pool, v_pool = pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv))
    i32 = R._i32
    plan = ops.shared_decode_plan([(0, 2)], [256], B, DEV)
    assert ops.decode_shared_supported(q.dtype, hs, N, dv) and ops.decode_rows_supported(q.dtype, hs, N, dv, ROWS_TQ)
    out = {
        "decode_paged": ops.diff_attention_decode_paged(q[:, 0], k_pool, v_pool, coef, table, i32(LENGTHS)),
        "decode_shared": ops.diff_attention_decode_paged_shared(q[:, 0], k_pool, v_pool, coef, table, i32(LENGTHS), plan),
        "extend_ragged_paged": ops.diff_attention_extend_paged(q, k_pool, v_pool, coef, table,
                                                               i32(STEPS["extend_ragged"][0])),
        "decode_rows_paged": ops.diff_attention_decode_rows_paged(q[:, :ROWS_TQ], k_pool, v_pool, coef, table,
                                                                  i32(STEPS["decode_rows"][0]), i32(ROWS_COUNTS)),
    }
    torch.cuda.synchronize()
    return {op: o.view(B, -1, H, dv) for op, o in out.items()}


def _fill_pages(pool, owner, k, v):
    P = pool.shape[1]
    for page, (b, r0) in owner.items():
        n = max(min(LENGTHS[b] - r0, P), 0)                    # rows past a length stay 0xFF (NaN)
        pool[page, :n] = torch.cat([k[b, r0:r0 + n].flatten(1), v[b, r0:r0 + n].flatten(1)], dim=-1)


@pytest.mark.parametrize("c", _far.cases("paged"), ids=_far.case_id)
def test_paged_cache(c):
    """diff_attention_decode_paged / _extend_paged / _decode_rows_paged / _decode_paged_shared on a
    bf16 pool that really is that large: the block table deals each sequence's pages across the
    near pages and the pages past 2^31 (and 2^32) bytes in turn.  The compact run is the same
    table shape over a pool of just those pages."""
    dtype, P = BF16, c.placement.shape[1]
    (q, k, v, coef), _ = _cache_compact("N2-hs64", dtype)
    ids, n_pages = _far.page_ids(2, P * c.placement.shape[2], c.distance, len(c.placement.ids))
    assert tuple(sorted(ids)) == c.placement.ids and n_pages == c.placement.shape[0]

    small = torch.full((len(ids) + 5, P, c.placement.shape[2]), -1, dtype=torch.int16, device=DEV).view(dtype)
    table, owner = _paged_table(P, [len(ids) + 1 - j for j in range(len(ids))])
    _fill_pages(small, owner, k, v)
    compact = _paged_run(small, table, q, coef, P)

    def body(fb):
        table, owner = _paged_table(P, ids)
        _fill_pages(fb.view, owner, k, v)
        far = _paged_run(fb.view, table, q, coef, P)
        fb.check()
        return far

    _check_steps("N2-hs64", dtype, _with_far(c, dtype, body), compact, _far.case_id(c))


# ------------------------------------------------------------------- row-wise kernels ---
LN_DT = {"x": F32, "y": BF16, "dy": BF16, "dx": F32, "res": BF16, "xo": F32, "dres": F32, "dx16": BF16}
assert {n: d.itemsize for n, d in LN_DT.items()} == _far.LN_ES and rw.COMBOS[_far.LN_COMBO] == (F32, BF16)


@functools.lru_cache(maxsize=None)
def _ln_problem(rows, C):
    return rw.ln_problem(_far.LN_COMBO, rows, C, 1e-5, 1.0, fused=True, seed=1)


def _ln_run(pb, far=None):
    """dta_ln_fwd / dta_ln_bwd of the add + LN fusion as test_gpu_rowwise_matrix's ``_run_direct``
    calls them, every operand packed but ``far`` = (name, view)."""
    lib = _lib.load()
    rows, C = pb.rows, pb.C
    t = {n: torch.full((rows, C), float("nan"), dtype=d, device=DEV) for n, d in LN_DT.items()}
    if far:
        t[far[0]] = far[1]
    for n, src in (("x", pb.x), ("dy", pb.dy), ("res", pb.res), ("dres", pb.dres)):
        t[n].copy_(src)
    w, b = pb.w.to(DEV), pb.b.to(DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    part = torch.empty(lib.dta_ln_bwd_workspace_bytes(rows, C) // 4, device=DEV)

    def ps(*names):
        return {k: v for n in names for k, v in ((n, t[n].data_ptr()), (n + "_stride", t[n].stride(0)))}

    a = RM._ln_args(pb, w=w.data_ptr(), b=b.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(), **ps("x", "y", "res", "xo"))
    _lib.check(lib.dta_ln_fwd(a, RM._stream()))
    a = RM._ln_args(pb, x=t["xo"].data_ptr(), x_stride=t["xo"].stride(0), w=w.data_ptr(), mean=mean.data_ptr(),
                    rstd=rstd.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(), partial=part.data_ptr(),
                    **ps("dy", "dx", "dres", "dx16"))
    _lib.check(lib.dta_ln_bwd(a, RM._stream()))
    torch.cuda.synchronize()
    return dict(y=t["y"].contiguous(), dx=t["dx"].contiguous(), xo=t["xo"].contiguous(), da=t["dx16"].contiguous(),
                dw=dw, db=db, mean=mean, rstd=rstd)


@functools.lru_cache(maxsize=None)
def _ln_compact(rows, C):
    return _ln_run(_ln_problem(rows, C))


def _rowwise_ln(c, fb):
    rows, C = c.placement.shape
    pb = _ln_problem(rows, C)
    got = _ln_run(pb, (c.operand, fb.view))
    fb.check()
    for name, want in _ln_compact(rows, C).items():
        assert torch.equal(got[name], want), (name, "differs from the packed rows' result")
        assert bool(torch.isfinite(got[name]).all()), name
    bad = {n: r.over[:4] for n, r in rw.judge_ln(pb, got).items() if r.over}          # test_gpu_rowwise_matrix's bars
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _swiglu_case():
    rows, n = _far.ROW_ROWS, _far.SWIGLU_N
    pb = rw.swiglu_problem(BF16, rows, n)
    return pb, _swiglu_run(pb, None)


def _swiglu_run(pb, far):
    rows, n = _far.ROW_ROWS, _far.SWIGLU_N
    t = {k: torch.full((rows, n), float("nan"), dtype=BF16, device=DEV) for k in _far.SWIGLU_OPERANDS}
    if far:
        t[far[0]] = far[1]
    for k, src in (("a", pb.a), ("b", pb.b), ("dout", pb.d)):
        t[k].copy_(src)
    RM._swiglu(BF16, rows, n, t["a"], t["b"], out=t["out"])
    RM._swiglu(BF16, rows, n, t["a"], t["b"], dout=t["dout"], da=t["da"], db=t["db"])
    torch.cuda.synchronize()
    return {k: t[k].contiguous() for k in ("out", "da", "db")}


def _rowwise_swiglu(c, fb):
    pb, compact = _swiglu_case()
    got = _swiglu_run(pb, (c.operand, fb.view))
    fb.check()
    for name, want in compact.items():
        assert torch.equal(got[name], want), (name, "differs from the packed rows' result")
        assert bool(torch.isfinite(got[name]).all()), name
        e = rw.elem_err(got[name].float(), pb.oracle[name], pb.aux[name], BF16)
        assert e < RM.TOL[BF16], (name, e)


def _rowwise_rope(c, fb):
    Bn, T, Hn, N, hs = _far.ROPE_SHAPE
    src64, ref = RM._rope_ref(Bn, T, Hn, N, hs, False)
    table = RM._freqs(hs, T)[1]
    src = src64.to(BF16).to(DEV)
    want = torch.full(src.shape, float("nan"), dtype=BF16, device=DEV)
    RM._rope(src, want, table, False)
    dst = torch.full(src.shape, float("nan"), dtype=BF16, device=DEV)
    if c.operand == "src":
        fb.view.copy_(src)
        RM._rope(fb.view, dst, table, False)
    else:
        dst = fb.view
        RM._rope(src, dst, table, False)
    torch.cuda.synchronize()
    got = dst.contiguous()
    fb.check()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert RM._rows_err(got, ref).max().item() < rw.ROPE_BAR[BF16]


def _rowwise_cast(c, fb):
    src = torch.randn(_far.ROPE_SHAPE, generator=torch.Generator().manual_seed(13)).to(DEV)
    RM._cast(src, fb.view)
    torch.cuda.synchronize()
    got = fb.view.contiguous()
    fb.check()
    RM._assert_same_bits(got, src.to(BF16), src)                # torch's one rounding: the reference and the packed result


@pytest.mark.parametrize("c", _far.cases("rowwise"), ids=_far.case_id)
def test_rowwise(c):
    """dta_ln_fwd / dta_ln_bwd (the add + LN fusion, fp32 stream and bf16 branch, C = 520 and
    3072), dta_swiglu_fwd / _bwd, dta_rope and dta_cast_f32 through the C ABI with one operand's
    row stride (rope and cast: also its batch stride) far; the rows from 20 on lie beyond (from 30
    for a 16-bit operand at far-4, where 20 would pass the memory cap).  far-8 (LN's fp32 x, 3
    rows 4 GiB apart): the sign-extended element image, 8 GiB below, is the one address not owned."""
    kind = c.key.split("-")[0]
    dtype = DTYPE[c.placement.es]
    _with_far(c, dtype, lambda fb: {"ln": _rowwise_ln, "swiglu": _rowwise_swiglu, "rope": _rowwise_rope,
                                    "cast": _rowwise_cast}[kind](c, fb))


# ------------------------------------------------------------------------ kv_quant_rows ---
def _quant_slots(pages):
    """Row (b, t) goes to row (8 + t) % P of sequence b's page (8 + t) // P."""
    P = _far.QUANT_P
    return [pages[2 * b + (8 + t) // P] * P + (8 + t) % P for b in range(_far.QUANT_B) for t in range(_far.QUANT_TN)]


def _quant_check(key, k_new, v_new, pool, scales, pages):
    """Every used page bitwise ``ops.kv_quant_reference`` on the host in the rows named by the
    slots and 0xFF everywhere else."""
    N, hs, dv = _far.QUANT[key]
    Hn, P = _far.QUANT_H, _far.QUANT_P
    kb, ks = ops.kv_quant_reference(k_new.cpu())
    vb, vs = ops.kv_quant_reference(v_new.cpu())
    rows = torch.cat([kb.flatten(2), vb.flatten(2)], dim=-1)                    # (B, Tn, W)
    sc = torch.cat([ks, vs[..., None]], dim=-1)                                 # (B, Tn, H, N + 1)
    want_b = {p: torch.full(pool.shape[1:], 0xFF, dtype=torch.uint8) for p in pages}
    want_s = {p: torch.full(scales.shape[1:], -1, dtype=torch.int32) for p in pages}
    for j, slot in enumerate(_quant_slots(pages)):
        b, t = divmod(j, _far.QUANT_TN)
        want_b[slot // P][slot % P] = rows[b, t]
        want_s[slot // P][slot % P] = sc[b, t].view(torch.int32)
    for p in pages:
        assert torch.equal(pool[p].cpu(), want_b[p]), (key, p, "bytes")
        assert torch.equal(scales[p].contiguous().view(torch.int32).cpu(), want_s[p]), (key, p, "scales")


def _quant_run(key, k_new, v_new, pool, scales, pages):
    N, hs, dv = _far.QUANT[key]
    nq = _far.QUANT_H * N * hs
    ops.kv_quant_rows(k_new, v_new, pool[..., :nq].unflatten(-1, (_far.QUANT_H, N, hs)),
                      pool[..., nq:].unflatten(-1, (_far.QUANT_H, dv)), scales, R._i32(_quant_slots(pages)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", _far.cases("quant"), ids=_far.case_id)
def test_kv_quant_rows(c):
    """kv_quant_rows with the destination slots in far pages -- a byte pool that is really that
    large and a scale pool on a far page stride, pages on both sides of the threshold -- or with
    k_new / v_new on a far batch stride, at (N 2, hs 128, dv 256: 32 lanes per item) and (N 3,
    hs 64, dv 128: 20 lanes), 164 items (a tail of 4).  Bitwise ``ops.kv_quant_reference`` on the
    host, which is also what the compact layout gives; every other byte of the pages 0xFF."""
    N, hs, dv = _far.QUANT[c.key]
    Bn, Tn, Hn, P = _far.QUANT_B, _far.QUANT_TN, _far.QUANT_H, _far.QUANT_P
    g = torch.Generator().manual_seed(7 * N + hs)
    k_new = (torch.randn(Bn, Tn, Hn, N, hs, generator=g) * 3).to(BF16).to(DEV)
    v_new = (torch.randn(Bn, Tn, Hn, dv, generator=g) * 3).to(BF16).to(DEV)
    W = Hn * (N * hs + dv)
    small = list(range(1, 1 + _far.quant_pages()))
    pool = torch.full((len(small) + 2, P, W), 0xFF, dtype=torch.uint8, device=DEV)
    scales = torch.full((len(small) + 2, P, Hn, N + 1), -1, dtype=torch.int32, device=DEV).view(F32)

    if c.operand == "pools":
        pages, n_pages = _far.page_ids(1, P * W, c.distance, _far.quant_pages(), between=False)
        assert tuple(sorted(pages)) == c.placement[0].ids and n_pages + 1 == c.placement[0].shape[0]

        def body(fb, fs):
            _quant_run(c.key, k_new, v_new, fb.view, fs.view, pages)
            _quant_check(c.key, k_new, v_new, fb.view, fs.view, pages)
            fb.check()
            fs.check()

        _with_far(c, (torch.uint8, F32), body)
    else:
        def body(fb):
            fb.view.copy_(k_new if c.operand == "k_new" else v_new)
            _quant_run(c.key, *((fb.view, v_new) if c.operand == "k_new" else (k_new, fb.view)), pool, scales, small)
            fb.check()

        _with_far(c, BF16, body)
        _quant_check(c.key, k_new, v_new, pool, scales, small)


# ---------------------------------------------------------------------- fp8 paged cache ---
FP8_OPS = {"decode_paged": "decode_ragged", "decode_shared": "decode_ragged", "extend_ragged_paged": "extend_ragged",
           "decode_rows_paged": "decode_rows"}


@functools.lru_cache(maxsize=None)
def _fp8_rows():
    """The logical caches of ``_cache_inputs`` quantised (``ops.kv_quant_reference``): the rows'
    bytes (B, CAP, W), their scales (B, CAP, H, N + 1) and the dequantised K / V in fp32."""
    q, k, v, coef = _cache_inputs("N2-hs64")
    kb, ks = ops.kv_quant_reference(k.to(BF16))
    vb, vs = ops.kv_quant_reference(v.to(BF16))
    kd = kb.view(torch.float8_e4m3fn).float() * ks[..., None]
    vd = vb.view(torch.float8_e4m3fn).float() * vs[..., None]
    return torch.cat([kb.flatten(2), vb.flatten(2)], -1), torch.cat([ks, vs[..., None]], -1), kd, vd


@functools.lru_cache(maxsize=None)
def _fp8_want(op):
    """``_cache_want`` on the dequantised rows (as test_gpu_fp8_cache's oracle) and bf16 q."""
    N, hs, dv = _far.CACHE["N2-hs64"]
    q, _, _, coef = _cache_inputs("N2-hs64")
    _, _, kd, vd = _fp8_rows()
    q, k, v = q.to(BF16).double(), kd.double(), vd.double()
    pos, counts = STEPS[op]
    want = torch.zeros(B, max(counts), H, dv, dtype=torch.float64)
    for b in range(B):
        n, L = counts[b], pos[b] + counts[b]
        for h in range(H):
            qs = []
            for i in range(N):
                rows = torch.zeros(1, L, hs, dtype=torch.float64)
                rows[0, pos[b]:] = q[b, :n, h, i]
                qs.append(rows)
            o = O.diff_core(qs, [k[b:b + 1, :L, h, i] for i in range(N)], v[b:b + 1, :L, h], coef[h].double())
            want[b, :n, h] = o[0, pos[b]:]
    return want


def _fp8_fill(pool, scales, owner):
    rows, sc, _, _ = _fp8_rows()
    P = pool.shape[1]
    for page, (b, r0) in owner.items():
        n = max(min(LENGTHS[b] - r0, P), 0)                    # rows past a length stay 0xFF: NaN bytes and scales
        pool[page, :n] = rows[b, r0:r0 + n].to(DEV)
        scales[page, :n] = sc[b, r0:r0 + n].to(DEV)


def _fp8_run(pool, scales, table, q, coef):
    N, hs, dv = _far.CACHE["N2-hs64"]
    nq = H * N * hs
    kp, vp = pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv))
    i32 = R._i32
    plan = ops.shared_decode_plan([(0, 2)], [256], B, DEV)
    assert ops.extend_fp8_supported(q.dtype, hs, N, dv) and ops.decode_shared_supported(q.dtype, hs, N, dv, fp8=True)
    assert ops.decode_rows_supported(q.dtype, hs, N, dv, ROWS_TQ, fp8=True)
    out = {
        "decode_paged": ops.diff_attention_decode_paged_fp8(q[:, 0], kp, vp, scales, coef, table, i32(LENGTHS)),
        "decode_shared": ops.diff_attention_decode_paged_shared_fp8(q[:, 0], kp, vp, scales, coef, table, i32(LENGTHS), plan),
        "extend_ragged_paged": ops.diff_attention_extend_paged_fp8(q, kp, vp, scales, coef, table,
                                                                   i32(STEPS["extend_ragged"][0])),
        "decode_rows_paged": ops.diff_attention_decode_rows_paged_fp8(q[:, :ROWS_TQ], kp, vp, scales, coef, table,
                                                                      i32(STEPS["decode_rows"][0]), i32(ROWS_COUNTS)),
    }
    torch.cuda.synchronize()
    return {op: o.view(B, -1, H, dv) for op, o in out.items()}


@pytest.mark.parametrize("c", _far.cases("fp8"), ids=_far.case_id)
def test_fp8_paged_cache(c):
    """The four fp8 twins (decode, extend, rows, shared-prefix decode on e4m3 pages) with a byte
    pool that really is past 2 GiB / 4 GiB and the scale pool's pages on a far
    ``scale_pool.stride(0)``; the table deals near and far pages in turn.  far-8: the scale pool
    alone (8 GiB; a far byte pool beside it would pass the memory cap), whose sign-extended element
    image, 8 GiB below, is the one address not owned.  The compact run is the same table shape
    over pools of just those pages; the oracle is fp64 on the dequantised rows."""
    P = _far.FP8_P
    (q, _, _, coef), _ = _cache_compact("N2-hs64", BF16)
    ids, n_pages, W = _far.fp8_ids(c.distance)
    places = _far.placements(c)
    assert all(tuple(sorted(ids)) == p.ids and p.shape[0] == n_pages for p in places)
    N = _far.CACHE["N2-hs64"][0]

    def small():
        return (torch.full((len(ids) + 5, P, W), 0xFF, dtype=torch.uint8, device=DEV),
                torch.full((len(ids) + 5, P, H, N + 1), -1, dtype=torch.int32, device=DEV).view(F32))

    pool, scales = small()
    table, owner = _paged_table(P, [len(ids) + 1 - j for j in range(len(ids))])
    _fp8_fill(pool, scales, owner)
    compact = _fp8_run(pool, scales, table, q, coef)

    def body(*fbs):
        table, owner = _paged_table(P, ids)
        if len(fbs) == 2:
            far_pool, far_scales = fbs[0].view, fbs[1].view
        else:                                                   # far-8: the byte pool small, with these page ids
            far_pool = torch.full((n_pages, P, W), 0xFF, dtype=torch.uint8, device=DEV)
            far_scales = fbs[0].view
        _fp8_fill(far_pool, far_scales, owner)
        far = _fp8_run(far_pool, far_scales, table, q, coef)
        for fb in fbs:
            fb.check()
        return far

    far = _with_far(c, (torch.uint8, F32) if len(places) == 2 else (F32,), body)
    for op, got in far.items():
        assert torch.equal(got, compact[op]), (op, "the far pools' result differs from the compact ones'")
        assert bool(torch.isfinite(got).all()), op
        step = FP8_OPS[op]
        want, counts = _fp8_want(step), STEPS[step][1]
        for b in range(B):
            err = rel_err(got[b, :counts[b]].float(), want[b, :counts[b]])
            assert err <= R.TOL[BF16], (op, b, err)
            assert bool((got[b, counts[b]:] == 0).all()), (op, b, "padding rows are zeros")
