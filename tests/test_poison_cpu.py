"""The poison harness (tests/_poison.py) must be able to fail: fake "kernels" written in torch
on the CPU, each with one of the defects the GPU poison tests look for, and a correct one.

A fake op allocates through ``torch.empty`` / ``torch.empty_like`` as ``ops.py`` does and
"launches" by writing through raw views, so the harness sees exactly what it would see of a
HIP kernel: the memory afterwards.
"""
import pytest
import torch

import _poison
from _poison import GUARD, poisoned_allocations

RESULTS = {"out", "stat"}
SCRATCH = {"work"}
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn]


def _raw(t, first, last):
    """Elements [first, last) relative to t's first element, bounds unchecked -- what a kernel's
    pointer arithmetic reaches (t is a view into a larger buffer under the harness)."""
    return t.as_strided((last - first,), (1,), t.storage_offset() + first)


def fake_scale(x, skip=None, before=False, after=False, extra=False, use_pad=None, pad_weight=1.0):
    """out = 2 x with a per-row partial-sum scratch ``work`` (one pad slot at the end, as the
    SwiGLU bias workspace has) and stat = sum(work[:rows]).  The keyword arguments plant defects:
    ``skip``: a flat index of ``out`` left unwritten; ``before`` / ``after``: a store one element
    outside ``out``; ``extra``: a further, unclassified allocation; ``use_pad``: "read" folds the
    never-written pad slot of ``work`` into stat, times ``pad_weight``."""
    rows = x.shape[0]
    out = torch.empty_like(x)
    work = torch.empty(rows + 1, device=x.device, dtype=torch.float32)
    stat = torch.empty(1, device=x.device, dtype=torch.float32)
    if extra:
        tmp = torch.empty(4, device=x.device, dtype=torch.float32)
        tmp.zero_()
    src = (2 * x.float()).to(x.dtype).view(-1)
    keep = torch.ones(src.numel(), dtype=torch.bool)
    if skip is not None:
        keep[skip] = False                                        # never stored: keeps what the allocation held
    out.view(-1)[keep] = src[keep]
    if before:
        _raw(out, -1, 0).fill_(1.0)
    if after:
        _raw(out, out.numel(), out.numel() + 1).fill_(1.0)
    work[:rows] = x.float().sum(-1)
    n = rows + 1 if use_pad == "read" else rows
    w = torch.ones(n)
    if use_pad == "read":
        w[-1] = pad_weight
    stat[0] = (work[:n] * w).sum()
    return out, stat


def _x(dtype=torch.float32, rows=5, n=7):
    g = torch.Generator().manual_seed(rows * n)
    return torch.randn(rows, n, generator=g).to(dtype)


# ------------------------------------------------------------------ mechanics ---
@pytest.mark.parametrize("dtype", DTYPES + [torch.int32, torch.uint8])
def test_allocation_is_poison_contiguous_aligned_and_recorded(dtype):
    with poisoned_allocations(cpu=True) as s:
        a = torch.empty(3, 5, dtype=dtype)
        b = torch.empty((2, 0, 4), dtype=dtype, device="cpu")
        c, d = torch.empty_like(a), torch.empty_like(a.t())
        z = torch.zeros(3, 5, dtype=dtype)                       # initialised by meaning: left alone
    assert [r.label for r in s.records] == ["test_allocation_is_poison_contiguous_aligned_and_recorded:" + n
                                            for n in "abcd"]
    assert a.is_contiguous() and a.shape == (3, 5) and a.dtype == dtype and b.shape == (2, 0, 4)
    assert c.is_contiguous() and d.stride() == a.t().stride()    # empty_like keeps a dense layout
    assert (z == 0).all() and len(s.records) == 4
    for t, r in zip((a, c, d), (s.records[0], s.records[2], s.records[3])):
        assert t.data_ptr() == r.base.data_ptr() + GUARD                     # GUARD keeps the alignment class
        assert (t.contiguous().view(torch.uint8) == 0xFF).all()
        if dtype.is_floating_point:
            assert t.float().isnan().all()
        else:
            assert (t.to(torch.int64) == (255 if dtype == torch.uint8 else -1)).all()
    for r in s.records:
        assert r.base.numel() == 2 * GUARD + r.nbytes and GUARD % 512 == 0
    s.check()


def test_gpu_only_by_default_and_torch_internals_untouched():
    with poisoned_allocations() as s:
        a = torch.empty(4)                                        # a CPU tensor, cpu=False
        torch.nn.Linear(3, 3)                                     # torch's own Python calls torch.empty
    assert s.records == [] and a.shape == (4,)
    with poisoned_allocations(cpu=True) as s:
        torch.nn.Linear(3, 3)
        torch.empty(2, dtype=torch.bool)
    assert s.records == []


def test_restored_after_an_exception_and_nested_blocks():
    orig, orig_like = torch.empty, torch.empty_like
    with pytest.raises(ZeroDivisionError):
        with poisoned_allocations(cpu=True):
            assert torch.empty is not orig
            with poisoned_allocations(cpu=True):
                1 / 0
    assert torch.empty is orig and torch.empty_like is orig_like
    with pytest.raises(RuntimeError):
        _poison.check()                                           # no block is active


def test_autograd_function_saves_a_poisoned_allocation():
    class Double(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty_like(x)
            out.copy_(2 * x)
            ctx.save_for_backward(out)
            return out.view(-1)

        @staticmethod
        def backward(ctx, g):
            (out,) = ctx.saved_tensors
            dx = torch.empty_like(out)
            dx.copy_(2 * g.view_as(out))
            return dx

    x = _x().requires_grad_(True)
    with poisoned_allocations(cpu=True) as s:
        y = Double.apply(x)
        y.sum().backward()
        s.verify({"out", "dx"}, set())
    assert torch.equal(y.detach(), 2 * x.detach().view(-1)) and torch.equal(x.grad, torch.full_like(x, 2.0))
    assert [r.label for r in s.records] == ["forward:out", "backward:dx"]


# ------------------------------------------------------------- a correct op ---
@pytest.mark.parametrize("dtype", DTYPES[:3])
def test_correct_op_passes_and_equals_the_unpoisoned_run(dtype):
    x = _x(dtype)
    plain = fake_scale(x)
    with poisoned_allocations(cpu=True) as s:
        got = fake_scale(_poison.guarded(x, "x"))
        s.verify(RESULTS, SCRATCH)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    assert s.names() == ["out", "work", "stat"] and s.names(allocated_only=False)[0] == "x"


# ------------------------------------------------------------ every defect ---
@pytest.mark.parametrize("dtype", DTYPES[:3])
@pytest.mark.parametrize("skip", [0, 17, 34])
def test_unwritten_output_element_is_reported(dtype, skip):
    x = _x(dtype)
    with poisoned_allocations(cpu=True) as s:
        fake_scale(x, skip=skip)
        s.check()
        with pytest.raises(AssertionError, match=r"fake_scale:out .*1 unwritten.*first at index \[%d, %d\]"
                           % divmod(skip, x.shape[1])):
            s.verify(RESULTS, SCRATCH)


@pytest.mark.parametrize("pad_weight", [1.0, 0.0])
def test_result_from_unwritten_scratch_is_reported(pad_weight):
    """A sum that folds in the never-written pad slot of ``work`` -- with weight 1, and with
    weight 0 (0 * garbage is 0 for any finite garbage; 0 * NaN is NaN)."""
    x = _x()
    with poisoned_allocations(cpu=True) as s:
        out, stat = fake_scale(x, use_pad="read", pad_weight=pad_weight)
        s.check()
        s.assert_classified(RESULTS, SCRATCH)
        assert torch.isfinite(out).all()
        with pytest.raises(AssertionError, match="fake_scale:stat"):
            s.assert_results_finite(RESULTS)
        # the scratch itself may keep its unwritten pad: a correct op passes with it unwritten
        assert s.records[1].name == "work" and s.records[1].tensor[-1].isnan()


@pytest.mark.parametrize("dtype", DTYPES[:3])
def test_store_before_the_start_and_past_the_end_is_reported(dtype):
    x = _x(dtype)
    es = x.element_size()
    with poisoned_allocations(cpu=True) as s:
        fake_scale(x, before=True)
        with pytest.raises(AssertionError, match=rf"fake_scale:out .*first at byte offset -{es} \({es} bytes before"):
            s.check()
    with poisoned_allocations(cpu=True) as s:
        fake_scale(x, after=True)
        with pytest.raises(AssertionError, match=r"fake_scale:out .*first at byte offset %d \(0 bytes past its end"
                           % (x.numel() * es)):
            _poison.check()
    with poisoned_allocations(cpu=True) as s:                     # a store past a caller's tensor
        g = _poison.guarded(x, "x")
        _raw(g, g.numel(), g.numel() + 1).fill_(0.0)
        with pytest.raises(AssertionError, match="guarded:x"):
            s.check()


def test_stale_but_plausible_buffer_cannot_pass_by_reuse():
    """An op that writes nothing: in a plain process its second call gets the first call's
    freed block back from a caching allocator and "returns" the right answer.  Under the
    harness no allocation is ever a reused one."""
    x = _x()
    state = {"launch": True}

    def op(x):
        out = torch.empty_like(x)
        if state["launch"]:
            out.copy_(2 * x)
        return out

    with poisoned_allocations(cpu=True) as s:
        first = op(x)
        s.verify({"out"}, set())
        state["launch"] = False
        del first
        second = op(x)
        assert s.records[0].base.data_ptr() != s.records[1].base.data_ptr()      # both buffers are kept alive
        assert second.isnan().all()
        with pytest.raises(AssertionError, match="op:out"):
            s.verify({"out"}, set())


def test_unclassified_allocation_is_reported():
    x = _x()
    with poisoned_allocations(cpu=True) as s:
        fake_scale(x, extra=True)
        with pytest.raises(AssertionError, match=r"neither.*fake_scale:tmp"):
            s.verify(RESULTS, SCRATCH)
        s.verify(RESULTS | {"tmp"}, SCRATCH)
        with pytest.raises(AssertionError, match="result and as scratch"):
            s.verify(RESULTS | {"tmp"}, SCRATCH | {"tmp"})


def test_arena_reports_stores_into_holes_and_guards():
    """``Arena``: hand-laid strided views of one poisoned buffer.  A padded layout's pad columns
    and the buffer's tail are holes; a store that ignores the row stride lands in one."""
    rows, cols, pad = 5, 16, 8
    st = cols + pad
    a = _poison.Arena(rows * st * 2, "cpu", "padded")
    v = a.view(torch.bfloat16, (rows, cols), (st, 1))
    assert a.holes() == rows * pad * 2 and v.isnan().all() and v.data_ptr() % 512 == a.base.data_ptr() % 512
    v.copy_(torch.ones(rows, cols))
    a.check()
    flat = a.base[GUARD:GUARD + a.nbytes].view(torch.bfloat16)
    flat[cols] = 1.0                                         # the packed position of row 1: a pad column here
    with pytest.raises(AssertionError, match=r"padded: 2 bytes .*payload byte offset 32 \(hole"):
        a.check()
    flat[cols] = v.new_tensor(float("nan")).view(torch.int16).fill_(-1).view(torch.bfloat16)
    a.check()
    a.base[GUARD + a.nbytes] = 0
    with pytest.raises(AssertionError, match="guard band past"):
        a.check()
    a.base[GUARD + a.nbytes] = 0xFF
    a.base[GUARD - 1] = 0
    with pytest.raises(AssertionError, match="guard band before"):
        a.check()


def test_arena_views_broadcast_overlap_and_bounds():
    a = _poison.Arena(64 * 4, "cpu")
    b = a.view(torch.float32, (3, 8), (0, 1), offset=4)      # a zero stride covers its elements once
    assert b.shape == (3, 8) and a.holes() == (64 - 8) * 4
    o = a.view(torch.float32, (4, 8), (6, 1), offset=16)     # rows overlapping by two elements (an input)
    assert a.holes() == (64 - 8 - 26) * 4 and o[0, 6:].data_ptr() == o[1, :2].data_ptr()
    with pytest.raises(AssertionError, match="view reaches"):
        a.view(torch.float32, (2, 8), (57, 1))
    a.check()
