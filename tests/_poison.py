"""Poisoned allocations with guard bands, for the tests of what the kernels write.

``torch.empty`` hands the kernels memory that, in a test process, is usually zero or the
previous call's (correct) result for the same shape, so an element a kernel never writes, a
read of scratch nobody wrote, and a store a few elements past a tensor all pass a max-norm
comparison.  Inside ``poisoned_allocations()`` every ``torch.empty`` / ``torch.empty_like`` made
by Python code outside the torch package (the wrappers of ``ops.py``, ``kv_cache.py`` and
``packing.py`` use no other uninitialised allocator) is instead the middle slice of a fresh
``uint8`` buffer filled with byte 0xFF, with ``GUARD`` bytes on each side:

* 0xFF.. is NaN in fp32, bf16, fp16 and e4m3fn and -1 in the integer types, so an element left
  unwritten, or anything computed from one (``0 * NaN`` included), is NaN in the result;
* every buffer is new and filled, so a stale but plausible value from an earlier call cannot
  stand in for a write;
* ``GUARD`` is a multiple of 512 bytes, so the slice keeps the allocator's alignment and 16-byte
  vector accesses behave as they do on a plain allocation;
* ``check()`` asserts that every guard byte is still 0xFF: a store before the start or past the
  end of a tensor is reported with its call site and byte offset.

``torch.zeros`` is left alone (initialised by meaning), and so are allocations made inside
torch's own C++ (a Python patch does not reach them) and by torch's own Python modules.

``guarded(t)`` copies a caller-made tensor (an input, dO, a cache, a pool, a table) into such a
buffer, so a store past a caller's tensor is seen too.

Each allocation is recorded with a label ``<function>:<variable>``, read from the calling frame
and its source line (``_DiffAttention.backward``'s ``dcp = torch.empty(...)`` is
``backward:dcp``); ``verify(results, scratch)`` is the order of checks the GPU tests use:
guards, then every allocation classified, then every result allocation finite.
"""
import contextlib
import linecache
import os
import re
import sys

import torch

GUARD = 4096                      # bytes on each side; a multiple of 512
FILL = 0xFF

_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_ACTIVE = []                      # the sessions in force, innermost last
_CALL = re.compile(r"torch\s*\.\s*empty(?:_like)?\s*\(")
_ASSIGN = re.compile(r"^\s*([A-Za-z_][\w\s,]*?)\s*=(?!=)")


class Record:
    """One poisoned allocation: ``base`` (uint8, guard | payload | guard), the payload's byte
    length, the tensor handed out and where it was asked for."""

    def __init__(self, base, nbytes, tensor, func, name):
        self.base, self.nbytes, self.tensor = base, nbytes, tensor
        self.shape, self.dtype = tuple(tensor.shape), tensor.dtype
        self.func, self.name = func, name

    @property
    def label(self):
        return f"{self.func}:{self.name}"

    def __repr__(self):
        return f"<{self.label} {self.dtype} {self.shape}>"


def _carve(nbytes, dtype, shape, strides, device):
    """(base, tensor): a fresh 0xFF buffer of GUARD + nbytes + GUARD bytes and its middle
    viewed as ``dtype`` with ``shape`` (contiguous unless ``strides`` says otherwise)."""
    base = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
    t = base[GUARD:GUARD + nbytes].view(dtype)
    t = t.view(shape) if strides is None else t.as_strided(shape, strides)
    return base, t


class Arena:
    """One poisoned buffer (guard | payload | guard, as ``_carve``) that a test lays strided
    views out in by hand -- the tensors of a C-ABI call at a layout of the test's choosing.

    ``view()`` hands out a view of the payload and records which payload bytes its elements
    cover; ``check()`` asserts that every guard byte and every *hole* byte (one no view covers:
    the pad columns of a padded row, the tail of a buffer) is still 0xFF, so a store that
    ignores a stride lands in memory the test owns and is reported."""

    def __init__(self, nbytes, device, label="arena"):
        self.nbytes, self.label = int(nbytes), label
        self.base = torch.full((GUARD + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.covered = torch.zeros(GUARD + self.nbytes + GUARD, dtype=torch.bool, device=device)

    def view(self, dtype, shape, strides, offset=0):
        """``shape`` / ``strides`` / ``offset`` in elements of ``dtype`` from the payload's start.
        A zero stride (a broadcast input) is allowed; the view must lie inside the payload."""
        es = dtype.itemsize
        shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
        assert offset >= 0 and all(s >= 0 for s in strides) and all(n > 0 for n in shape)
        reach = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
        assert reach * es <= self.nbytes, f"{self.label}: view reaches {reach * es} of {self.nbytes} bytes"
        t = self.base[GUARD:GUARD + self.nbytes].view(dtype).as_strided(shape, strides, GUARD // es + offset)
        once = tuple(1 if s == 0 else n for n, s in zip(shape, strides))
        self.covered.as_strided(once + (es,), tuple(s * es for s in strides) + (1,), GUARD + offset * es).fill_(True)
        return t

    def holes(self):
        """Number of payload bytes no view covers."""
        return int((~self.covered[GUARD:GUARD + self.nbytes]).sum())

    def check(self):
        """Every byte outside the views' elements is still 0xFF (synchronise first)."""
        bad = (self.base != FILL) & ~self.covered
        if not bool(bad.any()):
            return
        first = int(bad.nonzero()[0]) - GUARD
        where = ("guard band before the payload" if first < 0 else
                 "guard band past the payload" if first >= self.nbytes else "hole between the views' elements")
        raise AssertionError(f"out-of-bounds store: {self.label}: {int(bad.sum())} bytes outside every view written, "
                             f"first at payload byte offset {first} ({where})")


def _assigned_name(frame):
    """The variable the allocation on the frame's current line is assigned to: the target of
    ``x = torch.empty(...)``, or the matching one of ``a, b = torch.empty(..), torch.empty(..)``
    (the calls of one line are told apart by their bytecode offsets).  Falls back to
    ``L<line>`` where the line has no plain assignment."""
    code, lineno = frame.f_code, frame.f_lineno
    text = ""
    for ln in range(lineno, max(lineno - 4, 0), -1):       # a call spread over lines: its first line
        cand = linecache.getline(code.co_filename, ln)
        if _CALL.search(cand):
            text, lineno = cand, ln
            break
    m = _ASSIGN.match(text)
    if not m:
        return f"L{frame.f_lineno}"
    targets = [s.strip() for s in m.group(1).split(",") if s.strip()]
    if len(targets) == 1:
        return targets[0]
    if len(_CALL.findall(text)) != len(targets):
        return "|".join(targets)
    seen = _ASSIGNED_OFFSETS.setdefault((code, lineno), [])
    if frame.f_lasti not in seen:
        seen.append(frame.f_lasti)
        seen.sort()
    return targets[min(seen.index(frame.f_lasti), len(targets) - 1)]


_ASSIGNED_OFFSETS = {}


class Session:
    def __init__(self, cpu):
        self.cpu = cpu
        self.records = []

    # ---- allocation -------------------------------------------------------------------
    def _wants(self, device, dtype):
        if dtype == torch.bool or not (dtype.is_floating_point or dtype.is_complex or dtype in _INT_TYPES):
            return False
        return device.type == "cuda" or (self.cpu and device.type == "cpu")

    def _add(self, base, nbytes, t, func, name):
        self.records.append(Record(base, nbytes, t, func, name))
        return t

    def _empty(self, orig, frame, args, kwargs):
        kw = dict(kwargs)
        dtype = kw.pop("dtype", None) or torch.get_default_dtype()
        device = kw.pop("device", None)
        device = torch.device(device) if device is not None else torch.get_default_device()
        requires_grad = kw.pop("requires_grad", False)
        fmt = kw.pop("memory_format", torch.contiguous_format)
        if kw.pop("layout", torch.strided) != torch.strided or kw.pop("pin_memory", False) or kw \
                or fmt != torch.contiguous_format or not self._wants(device, dtype):
            return orig(*args, **kwargs)
        size = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)) else args
        size = tuple(int(s) for s in size)
        n = 1
        for s in size:
            n *= s
        base, t = _carve(n * dtype.itemsize, dtype, size, None, device)
        t = self._add(base, n * dtype.itemsize, t, frame.f_code.co_name, _assigned_name(frame))
        return t.requires_grad_() if requires_grad else t

    def _empty_like(self, orig, frame, args, kwargs):
        kw = dict(kwargs)
        src = args[0] if args else kw.pop("input")
        dtype = kw.pop("dtype", None) or src.dtype
        device = torch.device(kw.pop("device", None) or src.device)
        requires_grad = kw.pop("requires_grad", False)
        fmt = kw.pop("memory_format", torch.preserve_format)
        if len(args) > 1 or kw.pop("layout", torch.strided) != torch.strided or kw.pop("pin_memory", False) or kw \
                or src.layout != torch.strided or not self._wants(device, dtype):
            return orig(*args, **kwargs)
        # shape and strides as torch.empty_like would choose them (dense; preserved order)
        proto = orig(src, dtype=dtype, device="meta", memory_format=fmt)
        nbytes = proto.numel() * dtype.itemsize
        base, t = _carve(nbytes, dtype, tuple(proto.shape), None if proto.is_contiguous() else proto.stride(), device)
        t = self._add(base, nbytes, t, frame.f_code.co_name, _assigned_name(frame))
        return t.requires_grad_() if requires_grad else t

    def guarded(self, t, name="input"):
        """A copy of ``t`` (same shape, dtype and device, contiguous) inside a guarded buffer.
        Views are not followed: guard the packed tensor and slice the copy."""
        t = t.detach()
        nbytes = t.numel() * t.element_size()
        base, g = _carve(nbytes, t.dtype, tuple(t.shape), None, t.device)
        g.copy_(t)
        return self._add(base, nbytes, g, "guarded", name)

    # ---- checks -----------------------------------------------------------------------
    def _sync(self):
        if any(r.base.is_cuda for r in self.records):
            torch.cuda.synchronize()

    def check(self):
        """Every guard byte of every recorded buffer is still 0xFF (after a synchronise)."""
        self._sync()
        if not self.records:
            return
        flags = torch.stack([((r.base[:GUARD] != FILL).any() | (r.base[GUARD + r.nbytes:] != FILL).any()).cpu()
                             for r in self.records])
        if not flags.any():
            return
        msgs = []
        for r, bad in zip(self.records, flags.tolist()):
            if not bad:
                continue
            touched = torch.cat([r.base[:GUARD], r.base[GUARD + r.nbytes:]]) != FILL
            first = int(touched.nonzero()[0])
            off = first - GUARD if first < GUARD else r.nbytes + (first - GUARD)
            where = (f"{-off} bytes before its start" if off < 0 else f"{off - r.nbytes} bytes past its end")
            msgs.append(f"{r.label} {r.dtype} {r.shape}: guard band written, {int(touched.sum())} bytes, "
                        f"first at byte offset {off} ({where})")
        raise AssertionError("out-of-bounds store: " + "; ".join(msgs))

    def names(self, allocated_only=True):
        return [r.name for r in self.records if not (allocated_only and r.func == "guarded")]

    def assert_classified(self, results, scratch):
        """Every allocation (``guarded`` copies aside) is named in exactly one of the lists."""
        both = set(results) & set(scratch)
        assert not both, f"listed as result and as scratch: {sorted(both)}"
        unknown = sorted({r.label for r in self.records
                          if r.func != "guarded" and r.name not in results and r.name not in scratch})
        assert not unknown, (f"allocations in neither the results nor the scratch list: {unknown}; "
                             "classify them by what their consumer reads")

    def assert_results_finite(self, results):
        """Every element of every result allocation is finite (floating types) or not the
        poison value -1 / 0xFF.. (integer types)."""
        self._sync()
        recs = [r for r in self.records if r.func != "guarded" and r.name in results and r.tensor.numel()]
        if not recs:
            return
        bad = [(~torch.isfinite(r.tensor) if r.dtype.is_floating_point or r.dtype.is_complex
                else r.tensor.view(torch.uint8) == FILL) for r in recs]
        if r_any := [i for i, f in enumerate(torch.stack([b.any().cpu() for b in bad]).tolist()) if f]:
            msgs = []
            for i in r_any:
                idx = bad[i].reshape(-1).nonzero().reshape(-1)
                first = [int(j) for j in torch.unravel_index(idx[0], recs[i].shape)] if recs[i].shape else []
                msgs.append(f"{recs[i].label} {recs[i].dtype} {recs[i].shape}: {idx.numel()} unwritten or "
                            f"poison-derived elements, first at index {first}")
            raise AssertionError("result left unwritten or computed from unwritten memory: " + "; ".join(msgs))

    def verify(self, results, scratch):
        """(a) guards intact, (b) every allocation classified and every result finite."""
        self.check()
        self.assert_classified(results, scratch)
        self.assert_results_finite(results)


_INT_TYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _outside_torch(frame):
    return not os.path.abspath(frame.f_code.co_filename).startswith(_TORCH_DIR)


@contextlib.contextmanager
def poisoned_allocations(cpu=False):
    """Within the block ``torch.empty`` / ``torch.empty_like`` on the GPU (and on the CPU with
    ``cpu=True``) are poisoned, guarded and recorded; yields the ``Session``.  Both are put back
    on the way out, whatever happened inside."""
    session = Session(cpu)
    orig_empty, orig_like = torch.empty, torch.empty_like

    def empty(*args, **kwargs):
        frame = sys._getframe(1)
        if not _outside_torch(frame):
            return orig_empty(*args, **kwargs)
        return session._empty(orig_empty, frame, args, kwargs)

    def empty_like(*args, **kwargs):
        frame = sys._getframe(1)
        if not _outside_torch(frame):
            return orig_like(*args, **kwargs)
        return session._empty_like(orig_like, frame, args, kwargs)

    torch.empty, torch.empty_like = empty, empty_like
    _ACTIVE.append(session)
    try:
        yield session
    finally:
        _ACTIVE.remove(session)
        torch.empty, torch.empty_like = orig_empty, orig_like


def _current():
    if not _ACTIVE:
        raise RuntimeError("no poisoned_allocations() block is active")
    return _ACTIVE[-1]


def guarded(t, name="input"):
    """``Session.guarded`` of the innermost active block."""
    return _current().guarded(t, name)


def check():
    """``Session.check`` of the innermost active block."""
    _current().check()
