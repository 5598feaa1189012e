"""Operands far from their base pointer, for the tests of the kernels' address arithmetic.

Every strided operand of the C ABI carries 64-bit element strides, and every kernel is meant to
form ``index * stride`` in 64 bits.  A single ``int`` or ``uint32_t`` temporary in such an
expression changes nothing while every offset fits 31 bits, which is where every other test
keeps them.  Here one dimension of one operand gets a stride (or, for a page pool, an index)
that puts part of the operand *far* from the base pointer handed to the library:

* far-2: the byte offset lies in (2^31, 2^32): a signed 32-bit byte offset goes wrong;
* far-4: the byte offset is above 2^32 (for 16-bit types the element offset is then above 2^31
  too): an unsigned 32-bit byte offset and a signed 32-bit element offset go wrong;
* far-8: an fp32 element offset above 2^31.

A kernel with such a defect uses, instead of the true address, one of four *wrong images*
(``wrong_images``): the byte offset truncated to 32 bits, unsigned or sign-extended, or the
element offset treated so before it is scaled by the element size.  ``Placement`` sizes one
buffer that holds the operand and every wrong image of every far element, up to ``REACH``
(4 GiB) *below* the base pointer, and ``FarBuffer`` allocates it filled with 0xFF
(``_poison``'s NaN / -1 pattern): a wrong address then reads NaN or writes into poison the test
checks afterwards, so an address defect is a failed assertion in memory the test owns.

The arithmetic is plain integers with the word size a parameter (``bits``), so
tests/test_far_cpu.py checks every placement the GPU module uses without allocating, and runs
fake ops on a model scaled down to 16-bit words.
"""
import bisect
import collections
import functools

GiB = 1 << 30
CAP = 10 * GiB                      # live bytes a far test may hold (buffer + compact operands + temporaries)
ALIGN = 4096                        # the base pointer's alignment inside the buffer, bytes
SLACK = 1 << 20                     # how far past its threshold the first far element is put, bytes
REACH = 1 << 32                     # bytes owned below a base pointer at the most (a 16-bit type's 2^31 elements)
FILL = 0xFF
DISTANCES = ("far-2", "far-4", "far-8")


def _wrap(x, bits, signed):
    x &= (1 << bits) - 1
    if signed and x >> (bits - 1):
        x -= 1 << bits
    return x


def wrong_images(offset_elems, es, bits=32):
    """Byte offsets (relative to the base pointer, possibly negative) a kernel would use for the
    element at ``offset_elems`` if it held the byte offset, or the element offset before scaling,
    in an unsigned or a signed ``bits``-bit temporary; those equal to the true offset left out."""
    true = offset_elems * es
    images = {_wrap(true, bits, False), _wrap(true, bits, True),
              _wrap(offset_elems, bits, False) * es, _wrap(offset_elems, bits, True) * es}
    return sorted(images - {true})


def band(offset_elems, es, bits=32):
    """'near', 'far-2', 'far-4' or 'far-8' (fp32 only) of an element offset."""
    byte = offset_elems * es
    if es == 4 and offset_elems > 1 << (bits - 1):
        return "far-8"
    if byte > 1 << bits:
        return "far-4"
    if byte > 1 << (bits - 1):
        return "far-2"
    return "near"


def threshold(distance, es, bits=32):
    """The byte offset a ``distance`` element has to lie above."""
    return {"far-2": 1 << (bits - 1), "far-4": 1 << bits, "far-8": es << (bits - 1)}[distance]


def far_stride(distance, es, first_far, unit, bits=32, slack=SLACK):
    """The smallest element stride, a multiple of ``unit`` elements, that puts index
    ``first_far`` (>= 1) of its dimension ``slack`` bytes past the threshold of ``distance``."""
    assert first_far >= 1 and (distance != "far-8" or es == 4)
    need = -(-(threshold(distance, es, bits) + slack) // (first_far * es))
    return -(-need // unit) * unit


class Placement(collections.namedtuple("Placement", "name es shape strides far_dim first_far distance bits ids")):
    """One operand: ``shape`` / ``strides`` in elements of ``es`` bytes.  A *block* is the
    sub-tensor at one index of dimension ``far_dim``; the block at index ``first_far`` is at
    ``distance``, those after it there or further, those before it nearer.  ``ids``: the indices
    of ``far_dim`` a test touches (a page pool, of which only some pages are used); None: all."""

    @property
    def used(self):
        return tuple(range(self.shape[self.far_dim])) if self.ids is None else self.ids

    @property
    def block_elems(self):
        return 1 + sum((n - 1) * s for d, (n, s) in enumerate(zip(self.shape, self.strides)) if d != self.far_dim)

    def block_offsets(self):
        """Element offset of each used block's first element."""
        return [i * self.strides[self.far_dim] for i in self.used]

    def legit(self):
        """Byte intervals [lo, hi) the op may touch (a block's holes included)."""
        return [(o * self.es, (o + self.block_elems) * self.es) for o in self.block_offsets()]

    def images(self):
        """Byte intervals [lo, hi) of every wrong image of every used block.  A block never
        contains a multiple of 2^(bits-1) (bytes or elements), so its elements' images are its
        first element's, shifted alike."""
        out = []
        for o in self.block_offsets():
            last = o + self.block_elems - 1
            shifts = [[w - x * self.es for w in wrong_images(x, self.es, self.bits)] for x in (o, last)]
            assert shifts[0] == shifts[1], f"{self.name}: a block straddles a {self.bits}-bit threshold"
            out += [(o * self.es + s, (last + 1) * self.es + s) for s in shifts[0]]
        return tuple(out)

    def out_of_reach(self):
        """The images further than ``REACH`` below the base pointer, which the buffer does not
        hold: only the sign-extended element offset of far-8 (2^31 fp32 elements = 8 GiB below;
        with the 8 GiB above it that is past ``CAP``)."""
        return [(a, b) for a, b in self.images() if a < -(REACH >> (32 - self.bits))]

    @property
    def below(self):
        """Bytes owned below the base pointer: down to the lowest wrong image within ``REACH``,
        a multiple of ALIGN."""
        lo = min([0] + [a for a, _ in self.images() if a >= -(REACH >> (32 - self.bits))])
        return -(lo // ALIGN) * ALIGN

    @property
    def above(self):
        """Bytes owned from the base pointer up: the operand (a pool: all of it) and every image."""
        whole = 1 + sum((n - 1) * s for n, s in zip(self.shape, self.strides))
        hi = max([whole * self.es] + [b for _, b in self.images()])
        return -(-hi // 8) * 8

    @property
    def nbytes(self):
        return self.below + self.above

    def bands(self):
        """Band of each used block (of its first element; a block does not straddle)."""
        return [band(o, self.es, self.bits) for o in self.block_offsets()]

    def verify(self):
        """What tests/test_far_cpu.py asserts of every placement, in integers: the blocks from
        ``first_far`` on are at the claimed distance or further, the first of them in that band,
        the blocks before it nearer and one of them near; every far block has a wrong image and every wrong image differs from the
        true address, lies in the owned buffer and outside everything the op may touch."""
        order = ("near",) + DISTANCES
        bands = dict(zip(self.used, self.bands()))
        want = order.index(self.distance)
        far = [i for i in self.used if i >= self.first_far]
        assert far and bands[far[0]] == self.distance, (self.name, bands)
        assert all(order.index(bands[i]) >= want for i in far), (self.name, bands)
        assert all(order.index(bands[i]) < want for i in self.used if i < self.first_far), (self.name, bands)
        assert "near" in bands.values(), f"{self.name}: no block on the near side"
        legit, images = self.legit(), self.images()
        for o, b in zip(self.block_offsets(), bands.values()):
            wrong = wrong_images(o, self.es, self.bits)
            assert o * self.es not in wrong and (b == "near") == (not wrong), (self.name, o, b)
        assert not self.out_of_reach() or self.distance == "far-8", f"{self.name}: an image below the owned buffer"
        legit.sort()
        ends = [b for _, b in legit]
        beyond, below, above = set(self.out_of_reach()), self.below, self.above
        for lo, hi in images:
            if (lo, hi) in beyond:
                continue
            assert -below <= lo and hi <= above, f"{self.name}: image [{lo}, {hi}) outside the owned buffer"
            j = bisect.bisect_right(ends, lo)                   # the first block that ends past lo
            assert j == len(legit) or hi <= legit[j][0], f"{self.name}: image [{lo}, {hi}) overlaps the operand's {legit[j]}"
        return True


Placement.images = functools.lru_cache(maxsize=None)(Placement.images)      # a placement is immutable and hashable


def outer(name, es, shape, far_dim, first_far, distance, bits=32, unit=None, slack=None):
    """The placement of a logical ``shape`` whose dimension ``far_dim`` is outermost in memory on
    a far stride, the other dimensions contiguous in their logical order beneath it."""
    strides, run = [0] * len(shape), 1
    for d in reversed(range(len(shape))):
        if d != far_dim:
            strides[d], run = run, run * shape[d]
    unit = unit or max(16 // es, 1) * 5            # 16-byte aligned (vector and LDS-DMA accesses), no power of two
    if slack is None:                              # past the threshold by more than the blocks a wrapped offset could land on
        slack = (SLACK >> (32 - bits)) + 2 * first_far * run * es
    strides[far_dim] = max(far_stride(distance, es, first_far, unit, bits, slack), -(-run // unit) * unit)
    return Placement(name, es, tuple(shape), tuple(strides), far_dim, first_far, distance, bits, None)


def pool(name, es, shape, ids, distance, bits=32, page_stride=None):
    """A contiguous page pool ``shape`` = (n_pages, ...) that is really that large, of which a
    test touches the pages ``ids``; the pool's top pages reach ``distance``.  ``page_stride``
    (elements): pages contiguous inside, that far apart (the fp8 scale pool, whose real size
    cannot reach 2^31)."""
    strides, run = [0] * len(shape), 1
    for d in reversed(range(len(shape))):
        strides[d], run = run, run * shape[d]
    if page_stride is not None:
        assert page_stride >= strides[0]
        strides[0] = page_stride
    ids = tuple(sorted(ids))
    assert ids[-1] < shape[0]
    first_far = min(i for i in ids if band(i * strides[0], es, bits) == distance)
    return Placement(name, es, tuple(shape), tuple(strides), 0, first_far, distance, bits, ids)


def page_ids(es, page_elems, distance, count, bits=32, between=True):
    """``count`` page ids spread round-robin over every band from 'near' to ``distance``
    (``between`` False: over 'near' and ``distance`` alone; each band's ids a little past its
    threshold, 7 apart), and the n_pages that holds them."""
    order = ("near", "far-2", "far-4")
    bands = order[:order.index(distance) + 1] if between else ("near", distance)
    start = {"near": 3}
    for b in bands[1:]:
        start[b] = -(-(threshold(b, es, bits) + SLACK * (1 if bits == 32 else 0)) // (page_elems * es)) + 4      # + 4: a wrapped far id falls between the near ids (3 + 7 j)
    ids = [start[bands[j % len(bands)]] + 7 * (j // len(bands)) for j in range(count)]
    return ids, max(ids) + 5


# ------------------------------------------------------------------------- on the device ---
class FarBuffer:
    """The owned, 0xFF-filled buffer of one placement on a device, and the operand's view of it.

    ``view`` is the strided tensor to hand to the library (its ``data_ptr()`` is the base
    pointer, ``below`` bytes into the buffer).  ``check()`` puts 0xFF back into the elements of
    the view (every element the op may have written, or the test filled) and then asserts the
    whole buffer is 0xFF, through an int64 view in chunks, so no temporary passes 128 MiB."""

    CHUNK = 1 << 27                  # int64 words per compare (1 GiB read, a 128 MiB mask)

    def __init__(self, placement, dtype, device):
        import torch
        assert dtype.itemsize == placement.es
        self.placement, self.nbytes = placement, placement.nbytes
        assert self.nbytes % 8 == 0 and placement.below % ALIGN == 0
        self.buf = torch.full((self.nbytes,), FILL, dtype=torch.uint8, device=device)
        self.view = self.buf.view(dtype).as_strided(placement.shape, placement.strides, placement.below // placement.es)

    def repoison(self):
        """0xFF back into every element of the operand (a pool: of its used pages)."""
        import torch
        ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.placement.es]
        raw = self.view.view(ints)
        for part in ([raw] if self.placement.ids is None else [raw[i] for i in self.placement.ids]):
            part.fill_(FILL if self.placement.es == 1 else -1)

    def check(self):
        import torch
        torch.cuda.synchronize()
        self.repoison()
        words = self.buf.view(torch.int64)
        for lo in range(0, words.numel(), self.CHUNK):
            bad = words[lo:lo + self.CHUNK] != -1
            if bool(bad.any()):
                at = (lo + int(bad.nonzero()[0])) * 8 - self.placement.below
                raise AssertionError(f"{self.placement.name}: bytes outside the operand's elements written, first "
                                     f"near byte offset {at} from the base pointer")

    def release(self):
        self.buf = self.view = None


def need(*nbytes):
    """Bytes a test holds live: its far buffers, plus the compare temporary and headroom."""
    total = sum(nbytes) + (1 << 28)
    assert total <= CAP, f"{total / GiB:.2f} GiB is past the {CAP // GiB} GiB a far test may hold"
    return total


def skip_unless_free(nbytes):
    """The only admitted skip: less free device memory than the test holds."""
    import pytest
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip(f"{free / GiB:.1f} GiB free, {nbytes / GiB:.1f} GiB needed")


# ------------------------------------------------------------------------------ the cases ---
# One list for tests/test_gpu_far_addresses.py (which runs them) and tests/test_far_cpu.py (which
# checks every placement in integers).  ``key`` names the shapes, ``operand`` the tensor made far,
# ``dim`` the dimension carrying the far stride: b / t / h, or page for a pool that is that large.
FarCase = collections.namedtuple("FarCase", "family key operand dim distance placement")

# training core (dta_attn_fwd / dta_attn_bwd): es, N, hs, dv, rope, p; B = 2, T = 70, H = 2
TRAIN = {"bf16-N2": (2, 2, 64, 128, False, 0.0), "bf16-N3-rope": (2, 3, 64, 128, True, 0.0),
         "f32-N2": (4, 2, 64, 128, False, 0.0), "bf16-N2-drop": (2, 2, 64, 128, False, 0.1)}
TRAIN_B, TRAIN_T, TRAIN_H = 2, 70, 2
TRAIN_ROW = 60                      # the first far row of a far row stride: keeps the 16-bit far-4 buffer under CAP
QLIKE = ("q", "k", "dq", "dk", "qrot", "krot")          # (b, t, h, i, d)
VLIKE = ("v", "do", "o", "dv")                          # (b, t, h, e); obr: (i, b, t, h, e), fp32


def train_shape(key, operand):
    """(es, logical shape, index of b / t / h in it) of a training-core operand."""
    es, N, hs, dv, _, _ = TRAIN[key]
    if operand == "obr":
        return 4, (N, TRAIN_B, TRAIN_T, TRAIN_H, dv), {"b": 1, "t": 2, "h": 3}
    shape = (TRAIN_B, TRAIN_T, TRAIN_H) + ((N, hs) if operand in QLIKE else (dv,))
    return es, shape, {"b": 0, "t": 1, "h": 2}


def _train_cases():
    out = []

    def add(key, operand, dim, distance):
        es, shape, dims = train_shape(key, operand)
        first = TRAIN_ROW if dim == "t" else 1
        out.append(FarCase("train", key, operand, dim, distance,
                           outer(f"{key}-{operand}-{dim}-{distance}", es, shape, dims[dim], first, distance)))

    for key, (es, N, hs, dv, rope, p) in TRAIN.items():
        for operand in ("q", "k", "v", "do", "o", "dq", "dk", "dv", "obr") + (("qrot", "krot") if rope else ()):
            for distance in ("far-2", "far-4"):
                add(key, operand, "b", distance)
    add("f32-N2", "k", "b", "far-8")
    for distance in ("far-2", "far-4"):
        for operand in ("k", "v", "dk"):                        # head-major: st < sh
            add("bf16-N2", operand, "h", distance)
        for operand in ("k", "v", "q", "do", "dq", "dk", "dv", "o"):
            add("bf16-N2", operand, "t", distance)
    return out


# contiguous KV cache (decode, decode_ragged, decode_rows, extend, extend_ragged): N, hs, dv;
# B = 3 sequences of CACHE_LENGTHS rows in a cache of CACHE_CAP, H = 2
CACHE = {"N2-hs64": (2, 64, 128), "N3-hs128": (3, 128, 256), "N2-hs40": (2, 40, 80)}      # the last: no split plan, decode only
CACHE_B, CACHE_H, CACHE_CAP, CACHE_TQ = 3, 2, 600, 33
CACHE_LENGTHS = (600, 257, 600)
CACHE_ROW = {"far-2": 300, "far-4": 520}                # first far row; 520: keeps the 16-bit far-4 buffer under CAP


def cache_shape(key, operand):
    N, hs, dv = CACHE[key]
    if operand == "q":                                          # the extend step's rows; decode takes row 0
        return (CACHE_B, CACHE_TQ, CACHE_H, N, hs)
    if operand == "o":                                          # likewise: decode writes row 0 of it
        return (CACHE_B, CACHE_TQ, CACHE_H, dv)
    return (CACHE_B, CACHE_CAP, CACHE_H) + ((N, hs) if operand == "k" else (dv,))


def _cache_cases():
    out = []

    def add(key, operand, dim, distance, es=2):
        first = CACHE_ROW[distance] if dim == "t" else CACHE_B - 1          # batch: the last sequence (600 rows) is far
        out.append(FarCase("cache", key, operand, dim, distance,
                           outer(f"{key}-{operand}-{dim}-{distance}", es, cache_shape(key, operand),
                                 {"b": 0, "t": 1}[dim], first, distance)))

    for key in CACHE:
        for distance in ("far-2", "far-4"):
            for operand in ("k", "v"):
                add(key, operand, "b", distance)
                add(key, operand, "t", distance)
            add(key, "q", "b", distance)
            add(key, "o", "b", distance)
    add("N2-hs64", "k", "b", "far-8", es=4)
    return out


# paged KV cache (decode_paged, extend_paged, decode_rows_paged, decode_paged_shared): one packed
# bf16 pool (n_pages, P, [K | V]) that is really that large; N, hs, dv of CACHE["N2-hs64"]
PAGED_P = (32, 256)
PAGED_CAP = 768                     # rows a table row spans


def paged_pages(P):
    """Pages the three sequences own: those of sequence 2's first 256 rows are sequence 0's
    (a shared prefix), so fewer than 3 * ceil(600 / P)."""
    per = [-(-L // P) for L in CACHE_LENGTHS]
    return per, sum(per) - 256 // P


def _paged_cases():
    N, hs, dv = CACHE["N2-hs64"]
    W = CACHE_H * N * hs + CACHE_H * dv
    out = []
    for P in PAGED_P:
        for distance in ("far-2", "far-4"):
            ids, n_pages = page_ids(2, P * W, distance, paged_pages(P)[1])
            out.append(FarCase("paged", f"P{P}", "pool", "page", distance,
                               pool(f"P{P}-pool-{distance}", 2, (n_pages, P, W), ids, distance)))
    return out


# row-wise kernels through the C ABI (dta_ln_fwd / _bwd, dta_swiglu_fwd / _bwd, dta_rope, dta_cast_f32):
# 37 rows, one operand's row stride (rope / cast: also its batch stride) far
ROW_ROWS = 37
LN_COMBO, LN_WIDTHS = "f32-bf16", (520, 3072)           # the add + LN fusion: x / dx / xo / dres fp32, y / dy / res / dx16 bf16
LN_ES = {"x": 4, "y": 2, "dy": 2, "dx": 4, "res": 2, "xo": 4, "dres": 4, "dx16": 2}
SWIGLU_N = 520
SWIGLU_OPERANDS = ("a", "b", "out", "dout", "da", "db")
ROPE_SHAPE = (2, ROW_ROWS, 2, 2, 64)                    # (B, T, H, N, hs), bf16


def row_first(es, distance):
    """First far row of 37: 20, or the lowest that keeps the buffer (4 GiB below a 16-bit far-4
    operand, 8 GiB up to a far-8 one) under CAP."""
    return 34 if distance == "far-8" else 30 if (es, distance) == (2, "far-4") else 20


def _rowwise_cases():
    out = []

    def add(key, operand, dim, distance, es, shape, far_dim):
        first = row_first(es, distance) if dim == "t" else 1
        out.append(FarCase("rowwise", key, operand, dim, distance,          # unit 40: the row-wise entry points want strides % 8
                           outer(f"{key}-{operand}-{dim}-{distance}", es, shape, far_dim, first, distance, unit=40)))

    for distance in ("far-2", "far-4"):
        for C in LN_WIDTHS:
            for operand, es in LN_ES.items():
                add(f"ln-C{C}", operand, "t", distance, es, (ROW_ROWS, C), 0)
        for operand in SWIGLU_OPERANDS:
            add("swiglu", operand, "t", distance, 2, (ROW_ROWS, SWIGLU_N), 0)
        for dim, far_dim in (("b", 0), ("t", 1)):
            for operand in ("src", "dst"):
                add("rope", operand, dim, distance, 2, ROPE_SHAPE, far_dim)
            add("cast", "dst", dim, distance, 2, ROPE_SHAPE, far_dim)
    # far-8 on 3 rows (4 GiB apart: no row in far-2, whose image 2 GiB below would pass CAP)
    out.append(FarCase("rowwise", f"ln-C{LN_WIDTHS[0]}-r3", "x", "t", "far-8",
                       outer(f"ln-C{LN_WIDTHS[0]}-r3-x-t-far-8", 4, (3, LN_WIDTHS[0]), 0, 2, "far-8", unit=40)))
    return out


# kv_quant_rows: H = 2, P = 32, B = 2 sequences of 41 new rows; N, hs, dv (lanes per item: 32, 20)
QUANT = {"N2-hs128": (2, 128, 256), "N3-hs64": (3, 64, 128)}
QUANT_B, QUANT_TN, QUANT_H, QUANT_P = 2, 41, 2, 32       # 164 (row, head) items: 20 workgroups of 8 and a tail of 4


def quant_pages():
    """Pages the new rows go to: 41 rows per sequence from row 8 of a page, 2 pages each."""
    return 2 * QUANT_B


def _quant_cases():
    out = []
    for key, (N, hs, dv) in QUANT.items():
        W = QUANT_H * (N * hs + dv)
        for distance in ("far-2", "far-4"):
            ids, n_pages = page_ids(1, QUANT_P * W, distance, quant_pages(), between=False)
            name = f"{key}-pools-page-{distance}"
            # the byte pool is really that large; the scale pool has the same pages on a far page stride
            sids = sorted(ids)
            first = min(i for i in sids if band(i * QUANT_P * W, 1) == distance)
            stride = far_stride(distance, 4, first, 4, slack=SLACK + 8 * QUANT_P * QUANT_H * (N + 1) * 4)
            out.append(FarCase("quant", key, "pools", "page", distance,
                               (pool(name + "-bytes", 1, (n_pages + 1, QUANT_P, W), ids, distance),
                                pool(name + "-scales", 4, (n_pages + 1, QUANT_P, QUANT_H, N + 1), ids, distance,
                                     page_stride=stride))))
            for operand, es_shape in (("k_new", (QUANT_B, QUANT_TN, QUANT_H, N, hs)), ("v_new", (QUANT_B, QUANT_TN, QUANT_H, dv))):
                out.append(FarCase("quant", key, operand, "b", distance,
                                   outer(f"{key}-{operand}-b-{distance}", 2, es_shape, 0, 1, distance)))
    return out


# fp8 paged cache (the four fp8 twins): a byte pool (n_pages, P, [K | V]) that is really that large
# and a scale pool (n_pages, P, H, N + 1) of the same pages on a far page stride; N, hs, dv of
# CACHE["N2-hs64"], P = 32.  far-8: the scales alone (their pool beside a 4 GiB byte pool would
# pass CAP), the byte pool small.
FP8_P = 32


def fp8_ids(distance):
    N, hs, dv = CACHE["N2-hs64"]
    W = CACHE_H * (N * hs + dv)
    count = paged_pages(FP8_P)[1]
    if distance == "far-8":
        return [(3 if j % 2 == 0 else 1001) + j for j in range(count)], 1001 + count + 2, W       # near and far in turn
    ids, n_pages = page_ids(1, FP8_P * W, distance, count, between=False)
    return ids, n_pages, W


def _fp8_cases():
    N, hs, dv = CACHE["N2-hs64"]
    out = []
    for distance in DISTANCES:
        ids, n_pages, W = fp8_ids(distance)
        sids = sorted(ids)
        per_page = FP8_P * CACHE_H * (N + 1)
        if distance == "far-8":                                 # the pages from 1001 on beyond 2^31 elements
            first = min(i for i in sids if i > 1000)
            places = ()
        else:
            first = min(i for i in sids if band(i * FP8_P * W, 1) == distance)
            places = (pool(f"fp8-bytes-{distance}", 1, (n_pages, FP8_P, W), ids, distance),)
        stride = far_stride(distance, 4, first, 4, slack=SLACK + 8 * per_page * 4)
        places += (pool(f"fp8-scales-{distance}", 4, (n_pages, FP8_P, CACHE_H, N + 1), ids, distance, page_stride=stride),)
        out.append(FarCase("fp8", f"P{FP8_P}", "pools" if len(places) == 2 else "scales", "page", distance, places))
    return out


FAMILIES = ("train", "cache", "paged", "fp8", "quant", "rowwise")


def placements(c):
    """The placements of a case (the quantiser's pools are two buffers)."""
    return c.placement if isinstance(c.placement, tuple) and not isinstance(c.placement, Placement) else (c.placement,)


def cases(family=None):
    every = _train_cases() + _cache_cases() + _paged_cases() + _fp8_cases() + _rowwise_cases() + _quant_cases()
    return [c for c in every if family in (None, c.family)]


def case_id(c):
    return f"{c.key}-{c.operand}-{c.dim}-{c.distance}"
