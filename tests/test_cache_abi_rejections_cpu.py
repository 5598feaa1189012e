"""One rejection table over the thirteen attention-cache entry points of the C ABI.

Every call here returns before any launch: it fails validation, or it is empty (``B == 0``, or
``Tq == 0`` for the extends), so fake aligned addresses stand in for device memory and no GPU is
needed.  The return code of a call that is wrong in two ways is part of the ABI (the order of the
checks is behaviour), so the table holds one case per check class and doubly-wrong cases for the
precedences include/diffattn.h and csrc/capi.hip promise:

* one-row decodes: dims -> no plan (UNSUPPORTED) -> length -> ``B*H == 0`` is OK -> operands;
  the shared-prefix forms check ``n_groups`` and the group pointers before the plan query;
* multi-row decodes: ``pos`` / ``count`` and the ``Tq`` range before everything else;
* paged forms: null / ``lengths`` / table arguments first, then (fp8) the scale pool, then the rest;
* extends: UNSUPPORTED before the position checks, those before ``Tq == 0`` is OK.

Where two faults return the same code the order cannot show in it (the fp8 scale pool after the
table, the ``Tq`` range before the dims: INVALID either way); such a case is then paired with a
fault that does tell: no plan (UNSUPPORTED) or an empty batch (OK) behind it.

The expected codes are those of the library as it was before the host layer's checks were merged
into shared helpers (the commit "Replay a speculative-decoding round as one HIP graph"): the table
was run against that build through ``DTA_LIB`` and passed unchanged.  They are constants of this
file, never read from the library under test.
"""
import pytest

from differential_transformer_replication_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -2

ENTRIES = {
    "dta_attn_decode": _lib.DecodeArgs,
    "dta_attn_decode_ragged": _lib.DecodeRaggedArgs,
    "dta_attn_decode_paged": _lib.DecodePagedArgs,
    "dta_attn_decode_paged_fp8": _lib.DecodePagedFp8Args,
    "dta_attn_decode_paged_shared": _lib.DecodePagedSharedArgs,
    "dta_attn_decode_paged_shared_fp8": _lib.DecodePagedSharedFp8Args,
    "dta_attn_decode_rows": _lib.DecodeRowsArgs,
    "dta_attn_decode_rows_paged": _lib.DecodeRowsPagedArgs,
    "dta_attn_decode_rows_paged_fp8": _lib.DecodeRowsPagedFp8Args,
    "dta_attn_extend": _lib.ExtendArgs,
    "dta_attn_extend_ragged": _lib.ExtendRaggedArgs,
    "dta_attn_extend_paged": _lib.ExtendPagedArgs,
    "dta_attn_extend_paged_fp8": _lib.ExtendPagedFp8Args,
}

BASE = 0x100000                     # fake device addresses, 64 KiB apart, 16-byte aligned, never dereferenced
H, N, HS, DV, CAP, P, TQ = 2, 2, 64, 128, 64, 64, 4
(Q, K, V, O_, COEF, WS, LENGTHS, POS, COUNT, TABLE, SCALES, MEMBERS, ROWS) = (BASE + (i << 16) for i in range(13))
SCALE_STRIDE = P * H * (N + 1)


def _fields(struct):
    return {name for name, _ in struct._fields_}


def _valid(struct):
    """A call every check passes (bf16, one sequence, a plan for every entry point): the cases change it."""
    f = _fields(struct)
    a = struct()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv, a.t_cap, a.scale = _lib.DTA_BF16, 1, H, N, HS, DV, CAP, 0.125
    k, v = ("k_pool", "v_pool") if "k_pool" in f else ("k_cache", "v_cache")
    a.q = _lib.DtaTensor(Q, TQ * H * N * HS, H * N * HS, N * HS, HS)
    a.o = _lib.DtaTensor(O_, TQ * H * DV, H * DV, DV, 0)
    setattr(a, k, _lib.DtaTensor(K, CAP * H * N * HS, H * N * HS, N * HS, HS))
    setattr(a, v, _lib.DtaTensor(V, CAP * H * DV, H * DV, DV, 0))
    a.coef = COEF
    for name, value in (("length", 40), ("Tq", TQ), ("workspace", WS), ("lengths_dev", LENGTHS), ("pos_dev", POS),
                        ("count_dev", COUNT), ("page_size", P), ("max_pages", CAP // P), ("n_pages", 4),
                        ("block_table_dev", TABLE), ("scale_pool_dev", SCALES), ("scale_page_stride", SCALE_STRIDE),
                        ("n_groups", 1), ("group_members_dev", MEMBERS), ("group_rows_dev", ROWS)):
        if name in f:
            setattr(a, name, value)
    return a


def _cases(struct):
    """(label, {field path: value}, expected code) for one entry point; a value of ``+n`` as a string
    adds n to the valid call's value."""
    f = _fields(struct)
    extend = "workspace" not in f
    rows = "Tq" in f and not extend
    paged, fp8, shared = "block_table_dev" in f, "scale_pool_dev" in f, "n_groups" in f
    k, v = ("k_pool", "v_pool") if paged else ("k_cache", "v_cache")
    no_plan = {"head_size": 12}                       # dims are fine; no entry point has a plan for it
    empty = {"B": 0}

    c = [("empty batch", empty, OK),
         ("empty batch, null operands", {**empty, "q.ptr": None, "o.ptr": None, "coef": None}, OK),
         ("no plan", no_plan, UNSUPPORTED),
         ("no plan, empty batch", {**no_plan, **empty}, UNSUPPORTED),
         ("bad dims, no plan", {"dtype": 3, **no_plan}, INVALID)]
    c += [(f"bad dims {name}={value}", {name: value}, INVALID)
          for name, value in (("dtype", 3), ("dtype", -1), ("B", -1), ("H", 0), ("n_terms", 0), ("head_size", 0),
                              ("dv", 0))]
    # each operand: null, off the 16-byte vector, a stride off it, a negative stride
    for t in ("q", "o", k, v):
        c += [(f"{t} null", {f"{t}.ptr": None}, INVALID), (f"{t} misaligned", {f"{t}.ptr": "+2"}, INVALID),
              (f"{t} row stride", {f"{t}.st": "+1"}, INVALID), (f"{t} head stride", {f"{t}.sh": "+1"}, INVALID),
              (f"{t} negative stride", {f"{t}.sb": -16}, INVALID)]
    c += [("q branch stride", {"q.si": "+1"}, INVALID), (f"{k} branch stride", {f"{k}.si": "+1"}, INVALID),
          ("coef null", {"coef": None}, INVALID)]
    if not extend:
        c += [("workspace null", {"workspace": None}, INVALID), ("workspace misaligned", {"workspace": "+4"}, INVALID)]

    if "length" in f:                                 # the one-row decodes
        c += [("length 0", {"length": 0}, INVALID), ("length past t_cap", {"length": CAP + 1}, INVALID),
              ("no plan, length 0", {**no_plan, "length": 0}, UNSUPPORTED),
              ("length 0, empty batch", {"length": 0, **empty}, INVALID),
              ("head size 136", {"head_size": 136}, UNSUPPORTED), ("dv 264", {"dv": 264}, UNSUPPORTED),
              # (a page of an fp8 scale pool must hold the scales of every branch: checked before the plan)
              ("5 branches", {"n_terms": 5, **({"scale_page_stride": P * H * 6} if fp8 else {})}, UNSUPPORTED)]
    if "lengths_dev" in f:
        c += [("lengths null", {"lengths_dev": None}, INVALID), ("lengths misaligned", {"lengths_dev": "+2"}, INVALID),
              ("lengths null, no plan", {"lengths_dev": None, **no_plan}, INVALID),
              ("lengths null, empty batch", {"lengths_dev": None, **empty}, INVALID)]
    if "Tq" in f:
        c += [("Tq -1", {"Tq": -1}, INVALID)]
        if "pos_dev" in f:                            # the ragged extends and the multi-row decodes
            c += [("count null, empty batch", {"count_dev": None, **empty}, OK),
                  ("pos null", {"pos_dev": None}, INVALID), ("pos misaligned", {"pos_dev": "+2"}, INVALID),
                  ("count misaligned", {"count_dev": "+2"}, INVALID),
                  ("pos null, no plan", {"pos_dev": None, **no_plan}, INVALID),
                  ("count misaligned, no plan", {"count_dev": "+2", **no_plan}, INVALID),
                  ("pos null, empty batch", {"pos_dev": None, **empty}, INVALID)]
            if not paged:                             # (a table's t_cap is max_pages * P: its own check)
                c += [("t_cap below Tq", {"t_cap": TQ - 1}, INVALID),
                      ("no plan, t_cap below Tq", {**no_plan, "t_cap": TQ - 1}, UNSUPPORTED),
                      ("t_cap below Tq, empty batch", {"t_cap": TQ - 1, **empty}, INVALID)]
    if rows:
        c += [("Tq 0", {"Tq": 0}, INVALID), ("Tq 9", {"Tq": 9}, INVALID),
              ("Tq 9, no plan", {"Tq": 9, **no_plan}, INVALID), ("Tq 9, empty batch", {"Tq": 9, **empty}, INVALID),
              ("Tq 9, bad dims", {"Tq": 9, "dtype": 3}, INVALID)]
    if extend:
        c += [("no rows", {"Tq": 0}, OK), ("no rows, null operands", {"Tq": 0, "q.ptr": None, "coef": None}, OK),
              ("no plan, no rows", {**no_plan, "Tq": 0}, UNSUPPORTED)]
    if "pos" in f:                                    # dta_attn_extend's host position
        c += [("pos -1", {"pos": -1}, INVALID), ("rows past t_cap", {"pos": CAP - TQ + 1}, INVALID),
              ("t_cap -1", {"t_cap": -1, "Tq": 0}, INVALID), ("no plan, pos -1", {**no_plan, "pos": -1}, UNSUPPORTED),
              ("pos -1, no rows", {"pos": -1, "Tq": 0}, INVALID), ("pos -1, empty batch", {"pos": -1, **empty}, INVALID)]
    if paged:
        c += [("page size 48", {"page_size": 48}, INVALID), ("page size 512", {"page_size": 512}, INVALID),
              ("max_pages * P != t_cap", {"max_pages": 2}, INVALID), ("t_cap != max_pages * P", {"t_cap": 2 * CAP}, INVALID),
              ("no pages", {"n_pages": 0}, INVALID), ("max_pages 0", {"max_pages": 0}, INVALID),
              ("table null", {"block_table_dev": None}, INVALID), ("table misaligned", {"block_table_dev": "+2"}, INVALID),
              ("table null, no plan", {"block_table_dev": None, **no_plan}, INVALID),
              ("page size 48, empty batch", {"page_size": 48, **empty}, INVALID),
              ("page size 48, q null, no plan", {"page_size": 48, "q.ptr": None, **no_plan}, INVALID)]
    if fp8:
        c += [("scale pool null", {"scale_pool_dev": None}, INVALID),
              ("scale pool misaligned", {"scale_pool_dev": "+2"}, INVALID),
              ("short scale stride", {"scale_page_stride": SCALE_STRIDE - 1}, INVALID),
              (f"{k} page stride % 16", {f"{k}.sb": "+8"}, INVALID), (f"{k} row stride % 16", {f"{k}.st": "+8"}, INVALID),
              (f"{v} page stride % 16", {f"{v}.sb": "+8"}, INVALID), (f"{v} row stride % 16", {f"{v}.st": "+8"}, INVALID),
              ("scale pool null, no plan", {"scale_pool_dev": None, **no_plan}, INVALID),
              ("short scale stride, empty batch", {"scale_page_stride": SCALE_STRIDE - 1, **empty}, INVALID),
              ("5 branches, their scales do not fit", {"n_terms": 5}, INVALID),
              ("pool stride % 16, no plan", {f"{v}.st": "+8", **no_plan}, INVALID)]
    if shared:
        c += [("n_groups -1", {"n_groups": -1}, INVALID),
              ("members null", {"group_members_dev": None}, INVALID),
              ("members misaligned", {"group_members_dev": "+2"}, INVALID),
              ("group rows null", {"group_rows_dev": None}, INVALID),
              ("group rows misaligned", {"group_rows_dev": "+2"}, INVALID),
              ("n_groups -1, no plan", {"n_groups": -1, **no_plan}, INVALID),
              ("members null, no plan", {"group_members_dev": None, **no_plan}, INVALID),
              ("n_groups -1, empty batch", {"n_groups": -1, **empty}, INVALID),
              ("no groups, null plan, empty batch",
               {"n_groups": 0, "group_members_dev": None, "group_rows_dev": None, **empty}, OK)]
    return c


def _apply(a, path, value):
    *outer, last = path.split(".")
    for name in outer:
        a = getattr(a, name)
    if isinstance(value, str):
        value = (getattr(a, last) or 0) + int(value)
    setattr(a, last, value)


TABLE_CASES = [(entry, label, changes, want) for entry, struct in ENTRIES.items() for label, changes, want in _cases(struct)]


def test_table_covers_every_cache_entry_point():
    cache_entries = {n for n in _lib.EXPORTS if n.startswith(("dta_attn_decode", "dta_attn_extend"))
                     and not n.endswith("_bytes")}
    assert cache_entries == set(ENTRIES) and len(ENTRIES) == 13
    labels = [(e, l) for e, l, _, _ in TABLE_CASES]
    assert len(labels) == len(set(labels))
    for _, label, changes, want in TABLE_CASES:      # no case may reach a launch: it is rejected, or it is empty
        assert want < 0 or changes.get("B") == 0 or changes.get("Tq") == 0, label


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_args(entry):
    assert getattr(_lib.load(), entry)(None, None) == INVALID


@pytest.mark.parametrize("entry,label,changes,want", TABLE_CASES, ids=[f"{e[9:]}-{l}" for e, l, _, _ in TABLE_CASES])
def test_rejection_table(entry, label, changes, want):
    a = _valid(ENTRIES[entry])
    for path, value in changes.items():
        _apply(a, path, value)
    assert getattr(_lib.load(), entry)(a, None) == want
