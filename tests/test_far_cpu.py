"""The far-address harness (tests/_far.py) in integers, and proof that it can fail.

* Every placement tests/test_gpu_far_addresses.py uses (the one list ``_far.cases()``): the far
  blocks lie in the claimed band, every wrong image differs from the true address, and every
  wrong image lies inside the owned, poisoned buffer and outside everything the op may touch.
  Pure integer arithmetic: nothing is allocated.
* Fake gather / scatter ops in NumPy on a model scaled to 16-bit words (thresholds 2^15 and
  2^16 bytes), each with one of the four address defects the harness exists to find, and a
  correct one: the four steps of the GPU tests -- bitwise against the compact run, finite, the
  after-check of the poison -- must report each defect and pass the correct op.
"""
import numpy as np
import pytest

import _far

BITS = 16
FAULTS = ["byte-u", "byte-s", "elem-u", "elem-s"]


# ------------------------------------------------------------------------ the placements ---
@pytest.mark.parametrize("c", _far.cases(), ids=lambda c: f"{c.family}:{_far.case_id(c)}")
def test_placement(c):
    places = _far.placements(c)
    assert _far.need(*[p.nbytes for p in places]) <= _far.CAP
    for p in places:
        assert p.verify()
        # the only images no buffer under CAP can hold: far-8's sign-extended element offset, 8 GiB below
        assert bool(p.out_of_reach()) == (c.distance == "far-8")
        for lo, _ in p.out_of_reach():
            assert lo < -7 * _far.GiB
        # the base pointer keeps the alignment of an allocation, the far stride that of a 16-byte access
        assert p.below % _far.ALIGN == 0 and (p.strides[p.far_dim] * p.es) % 16 == 0
    if c.family == "paged":                                      # pages on both sides of each threshold
        order = ("near",) + _far.DISTANCES
        assert set(places[0].bands()) == set(order[:order.index(c.distance) + 1])


# the families of kernels with strided operands, and the distances each is to reach
WANTED = {"train": _far.DISTANCES, "cache": _far.DISTANCES, "paged": ("far-2", "far-4"), "fp8": _far.DISTANCES,
          "quant": ("far-2", "far-4"), "rowwise": _far.DISTANCES}


def test_every_family_reaches_every_distance():
    seen = {(c.family, c.distance) for c in _far.cases()}
    assert seen == {(f, d) for f, ds in WANTED.items() for d in ds}
    ids = [(c.family, _far.case_id(c)) for c in _far.cases()]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("es", [1, 2, 4])
def test_wrong_images(es):
    """The four truncations by hand at the edges of each band."""
    assert _far.wrong_images((1 << 31) // es, es) == [-(1 << 31)]          # exactly 2^31 bytes: only the signed byte offset
    assert _far.wrong_images((1 << 31) // es - 1, es) == []
    e = (1 << 32) // es + 3
    want = {3 * es} | ({(e - (1 << 32)) * es} if es == 2 else set())       # 16-bit: 2^31 + 3 elements sign-extend
    assert set(_far.wrong_images(e, es)) == want
    assert _far.band(e, es) == "far-4" and _far.band((1 << 31) // es + 1, es) == "far-2"
    if es == 4:
        e = (1 << 31) + 5
        assert _far.band(e, 4) == "far-8"
        assert set(_far.wrong_images(e, 4)) == {20, (e - (1 << 32)) * 4}


# ------------------------------------------------------------------------------ fake ops ---
ES = 2
ROWS = (5, 8)                                         # a block: rows, columns


def _placement(distance, blocks=2):
    return _far.outer(f"fake-{distance}-{blocks}", ES, (blocks,) + ROWS, 0, 1, distance, bits=BITS, unit=8)


def _address(offset_elems, fault):
    """Byte offset from the base pointer as a kernel with ``fault`` forms it."""
    if fault == "byte-u":
        return _far._wrap(offset_elems * ES, BITS, False)
    if fault == "byte-s":
        return _far._wrap(offset_elems * ES, BITS, True)
    if fault == "elem-u":
        return _far._wrap(offset_elems, BITS, False) * ES
    if fault == "elem-s":
        return _far._wrap(offset_elems, BITS, True) * ES
    return offset_elems * ES


class FakeBuffer:
    """``_far.FarBuffer`` in NumPy: 0xFF everywhere, the base pointer ``below`` bytes in."""

    def __init__(self, placement):
        self.p = placement
        self.buf = np.full(placement.nbytes, _far.FILL, dtype=np.uint8)

    def _at(self, index, fault=None):
        off = sum(i * s for i, s in zip(index, self.p.strides))
        at = self.p.below + _address(off, fault)
        assert 0 <= at and at + ES <= self.buf.size, "an address outside the owned buffer"
        return at

    def store(self, index, value, fault=None):
        at = self._at(index, fault)
        self.buf[at:at + ES] = np.frombuffer(np.float16(value).tobytes(), dtype=np.uint8)

    def load(self, index, fault=None):
        at = self._at(index, fault)
        return np.frombuffer(self.buf[at:at + ES].tobytes(), dtype=np.float16)[0]

    def check(self):
        """As ``FarBuffer.check``: 0xFF back into the operand's elements, then all of it 0xFF."""
        for index in np.ndindex(*self.p.shape):
            at = self._at(index)
            self.buf[at:at + ES] = _far.FILL
        bad = np.flatnonzero(self.buf.view(np.int64) != -1)
        assert bad.size == 0, f"bytes outside the operand's elements written, first near {bad[0] * 8 - self.p.below}"


def _values(shape):
    return np.random.default_rng(5).standard_normal(shape).astype(np.float16)


def fake_gather(src, fault=None):
    """out = 2 src, the source read at a kernel's addresses."""
    out = np.empty(src.p.shape, dtype=np.float16)
    for index in np.ndindex(*out.shape):
        out[index] = np.float16(2) * src.load(index, fault)
    return out


def fake_scatter(x, dst, fault=None):
    """dst = 2 x, the destination written at a kernel's addresses."""
    for index in np.ndindex(*x.shape):
        dst.store(index, np.float16(2) * x[index], fault)


def _harness(op, placement, fault):
    """The GPU tests' steps on a fake op; raises AssertionError as they do."""
    shape = placement.shape
    x = _values(shape)
    compact = np.float16(2) * x
    fb = FakeBuffer(placement)
    if op == "gather":
        for index in np.ndindex(*shape):
            fb.store(index, x[index])
        far = fake_gather(fb, fault)
    else:
        fake_scatter(x, fb, fault)
        far = np.array([fb.load(index) for index in np.ndindex(*shape)], dtype=np.float16).reshape(shape)
    assert np.array_equal(far.view(np.uint16), compact.view(np.uint16)), "the far result differs from the compact one"
    assert np.isfinite(far).all(), "unwritten or poison-derived elements"
    fb.check()


# (distance of block 1, blocks) -> the faults that change an address there.  es = 2: a far-4 byte
# offset's element offset is past the signed 16-bit range but fits the unsigned one; the third
# block of a far-4 stride lies past 2^17 bytes, where the unsigned element offset wraps too.
EXPECT = {("far-2", 2): {"byte-s"}, ("far-4", 2): {"byte-u", "byte-s", "elem-s"}, ("far-4", 3): set(FAULTS)}


@pytest.mark.parametrize("distance,blocks", list(EXPECT))
@pytest.mark.parametrize("op", ["gather", "scatter"])
def test_the_faultless_op_passes(op, distance, blocks):
    p = _placement(distance, blocks)
    assert p.verify() and p.nbytes < 1 << 20
    _harness(op, p, None)


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("op", ["gather", "scatter"])
def test_each_fault_is_reported(op, fault):
    """Every defect is reported wherever it changes an address (and nowhere else: there it
    forms the true address, which no layout can show), and each of the four somewhere."""
    reported = set()
    for (distance, blocks), faults in EXPECT.items():
        p = _placement(distance, blocks)
        assert (fault in faults) == any(_address(o, fault) != o * ES for o in p.block_offsets())
        try:
            _harness(op, p, fault)
        except AssertionError:
            reported.add((distance, blocks))
    assert reported == {key for key, faults in EXPECT.items() if fault in faults} and reported


def test_far_8_model():
    """fp32-like elements (es = 4) on the scaled model: far-8's sign-extended element image is
    the one left out of the buffer, every other image is owned."""
    p = _far.outer("fake-far-8", 4, (2,) + ROWS, 0, 1, "far-8", bits=BITS, unit=4)
    assert p.verify() and len(p.out_of_reach()) == 1
    assert p.out_of_reach()[0][0] < -(4 << (BITS - 1)) + p.strides[0] * 4
