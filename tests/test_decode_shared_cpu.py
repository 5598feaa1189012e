"""Host side of the shared-prefix decode (no GPU): the ctypes structs against the header, the
export list, the argument checks of the two entry points (at B = 0, so no pointer is
dereferenced and nothing is launched), the capability check, the host planner on hand-built
allocator state and the dispatch of ``shared_decode``."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "dta_attn_decode_paged_shared_args": _lib.DecodePagedSharedArgs,
    "dta_attn_decode_paged_shared_fp8_args": _lib.DecodePagedSharedFp8Args,
}
PLAN = ["n_groups", "group_members_dev", "group_rows_dev"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_shared_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    # sizeof of a call is not evaluated: nothing links, and an undeclared or differently typed
    # function does not compile
    lines += ['  printf("symbols declared %zu\\n", sizeof(dta_attn_decode_paged_shared((const dta_attn_decode_paged_shared_args*)0, (void*)0))'
              ' / sizeof(dta_attn_decode_paged_shared_fp8((const dta_attn_decode_paged_shared_fp8_args*)0, (void*)0))'
              ' * sizeof(dta_decode_shared_supported(0, 0, 0, 0, 0)) / sizeof(int));',
              '  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-Werror=implicit-function-declaration", "-I", os.path.join(ROOT, "include"),
                        src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    assert got[("abi", "version")] == _lib.ABI_VERSION == 9         # the feature arrives without an ABI bump
    assert got[("symbols", "declared")] == 1
    bad = []
    for cname, py in STRUCTS.items():
        if got[(cname, "sizeof")] != ctypes.sizeof(py):
            bad.append((cname, "sizeof", got[(cname, "sizeof")], ctypes.sizeof(py)))
        for f in py._fields_:
            off = getattr(py, f[0]).offset
            if got[(cname, f[0])] != off:
                bad.append((cname, f[0], got[(cname, f[0])], off))
    assert not bad, bad
    # the paged and the fp8 paged decode structs with the plan appended
    names = lambda py: [f[0] for f in py._fields_]
    assert names(_lib.DecodePagedArgs) + PLAN == names(_lib.DecodePagedSharedArgs)
    assert names(_lib.DecodePagedFp8Args) + PLAN == names(_lib.DecodePagedSharedFp8Args)


def test_shared_exports():
    assert _lib.SHARED_EXPORTS == ("dta_attn_decode_paged_shared", "dta_attn_decode_paged_shared_fp8",
                                   "dta_decode_shared_supported")
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    for name in _lib.SHARED_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert _lib.shared_symbols(lib)

    class _Old:                                   # a library of the same ABI without the symbols
        dta_attn_decode_paged = dta_attn_decode_paged_fp8 = dta_attn_decode_rows_paged = None
    assert not _lib.shared_symbols(_Old())


def _args(cls=_lib.DecodePagedSharedFp8Args, **kw):
    """A call that passes every host check at B = 0."""
    a = cls()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 2, 2, 64, 128
    a.length, a.t_cap, a.scale = 100, 128, 0.125
    buf = (ctypes.c_int32 * 16)()
    a._keep = buf
    a.lengths_dev = a.block_table_dev = ctypes.addressof(buf)
    a.page_size, a.max_pages, a.n_pages = 64, 2, 4
    a.k_pool.sb, a.k_pool.st, a.k_pool.sh, a.k_pool.si = 64 * 512, 512, 128, 64
    a.v_pool.sb, a.v_pool.st, a.v_pool.sh = 64 * 512, 512, 128
    if cls is _lib.DecodePagedSharedFp8Args:
        a.scale_pool_dev = ctypes.addressof(buf)
        a.scale_page_stride = 64 * 2 * 3
    a.n_groups = 1
    a.group_members_dev = a.group_rows_dev = ctypes.addressof(buf)
    for k, v in kw.items():
        obj = a
        *path, leaf = k.split("__")
        for name in path:
            obj = getattr(obj, name)
        setattr(obj, leaf, v)
    return a


def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    entries = ((lib.dta_attn_decode_paged_shared, _lib.DecodePagedSharedArgs),
               (lib.dta_attn_decode_paged_shared_fp8, _lib.DecodePagedSharedFp8Args))
    for fn, cls in entries:
        call = lambda **kw: fn(ctypes.byref(_args(cls, **kw)), None)
        base = _args(cls).lengths_dev
        assert fn(None, None) == -1
        assert fn(ctypes.byref(cls()), None) == -1
        assert call() == 0                                           # B = 0: valid, no launch
        assert call(n_groups=0) == 0
        assert call(n_groups=0, group_members_dev=None, group_rows_dev=None) == 0    # G = 0 needs no plan pointers
        assert call(n_groups=-1) == -1
        assert call(group_members_dev=None) == -1 and call(group_rows_dev=None) == -1
        assert call(group_members_dev=base + 2) == -1 and call(group_rows_dev=base + 1) == -1
        assert call(group_members_dev=base + 4, group_rows_dev=base + 8) == 0
        assert call(lengths_dev=None) == -1 and call(lengths_dev=base + 2) == -1
        assert call(block_table_dev=None) == -1 and call(block_table_dev=base + 2) == -1
        assert call(dtype=3) == -1 and call(B=-1) == -1 and call(H=0) == -1
        assert call(length=0) == -1 and call(length=129) == -1
        assert call(t_cap=127) == -1 and call(max_pages=3) == -1     # t_cap != max_pages * page_size
        assert call(page_size=48, max_pages=2, t_cap=96) == -1
        assert call(page_size=32, max_pages=4, scale_page_stride=32 * 6) == 0
        assert call(n_pages=0) == -1
        for bad in (dict(head_size=40, dv=80), dict(head_size=16, dv=32), dict(n_terms=5), dict(dv=64), dict(head_size=132)):
            if "n_terms" in bad:
                bad["scale_page_stride"] = 64 * 2 * 6
            assert call(**bad) == -2, bad                            # no split plan: unsupported, no other kernel
        assert call(n_terms=1, dv=64) == 0
    call = lambda **kw: entries[1][0](ctypes.byref(_args(**kw)), None)
    assert call(scale_pool_dev=None) == -1
    assert call(scale_pool_dev=_args().scale_pool_dev + 2) == -1
    assert call(scale_page_stride=64 * 2 * 3 - 1) == -1
    for field in ("k_pool__sb", "k_pool__st", "v_pool__sb", "v_pool__st"):
        assert call(**{field: 520}) == -1, field                     # 520 % 16 == 8
        assert call(**{field: 528}) == 0, field


def test_capability():
    lib = _lib.load()
    for fp8 in (0, 1):
        for dtype in (0, 1, 2):
            for hs, dv in ((32, 64), (64, 128), (128, 256)):
                for n in (1, 2, 3, 4):
                    assert lib.dta_decode_shared_supported(dtype, hs, n, dv, fp8) == 1
                    assert lib.dta_decode_shared_supported(dtype, hs, n, dv, fp8) == lib.dta_decode_rows_supported(dtype, hs, n, dv, 1, fp8)
            assert lib.dta_decode_shared_supported(dtype, 64, 1, 64, fp8) == 1
            assert lib.dta_decode_shared_supported(dtype, 128, 1, 128, fp8) == 1
            assert lib.dta_decode_shared_supported(dtype, 64, 2, 64, fp8) == 0
            assert lib.dta_decode_shared_supported(dtype, 64, 5, 128, fp8) == 0
            assert lib.dta_decode_shared_supported(dtype, 64, 0, 128, fp8) == 0
            assert lib.dta_decode_shared_supported(dtype, 16, 2, 32, fp8) == 0
            assert lib.dta_decode_shared_supported(dtype, 40, 2, 80, fp8) == 0
        assert lib.dta_decode_shared_supported(3, 64, 2, 128, fp8) == 0
        assert lib.dta_decode_shared_supported(-1, 64, 2, 128, fp8) == 0
    assert ops.decode_shared_supported(torch.bfloat16, 64, 2, 128) and ops.decode_shared_supported(torch.float32, 64, 2, 128, fp8=True)
    assert not ops.decode_shared_supported(torch.bfloat16, 40, 2, 80)
    # the one-row workspace serves the new entry points: its size is what it was
    assert lib.dta_attn_decode_workspace_bytes(3, 2, 2, 64, 128, 768) == max(3 * 2 * 2 * 768 * 4, 3 * 2 * 3 * 2 * 130 * 4)


# ------------------------------------------------------------- plan object ---
def test_plan_validation_and_upload():
    plan = ops.shared_decode_plan([(0, 2, 3), (4, 1)], [544, 256], 5, "cpu")
    assert plan.n_groups == 2 and plan.B == 5
    assert plan.members.dtype == torch.int32 and plan.rows.dtype == torch.int32
    assert plan.members.tolist() == [[0, 2, 3, -1, -1, -1, -1, -1], [4, 1, -1, -1, -1, -1, -1, -1]]
    assert plan.rows.tolist() == [544, 256]
    assert plan.members.is_contiguous() and plan.members.data_ptr() % 4 == 0 and plan.rows.data_ptr() % 4 == 0
    empty = ops.shared_decode_plan([], [], 5, "cpu")
    assert empty.n_groups == 0 and empty.members is None and empty.rows is None
    for groups, rows in (([(0,)], [300]), ([tuple(range(9))], [300]), ([(0, 5)], [300]), ([(0, -1)], [300]),
                         ([(0, 0)], [300]), ([(0, 1), (1, 2)], [300, 300]), ([(0, 1)], [-1]), ([(0, 1)], [300, 300])):
        with pytest.raises(ValueError):
            ops.shared_decode_plan(groups, rows, 5 if len(groups[0]) < 9 else 16, "cpu")


# ----------------------------------------------------------------- planner ---
P = 32


def _cache(lists, low, **kw):
    """A PagedKVCache whose allocator state is written by hand: sequence q holds ``lists[q]``."""
    cache = kv_cache.PagedKVCache(64, P, **kw)
    for q, pages in enumerate(lists):
        cache.pages[q] = list(pages)
        cache.host_lengths[q] = cache.host_low[q] = low[q]
    return cache


def test_planner_two_forks_of_one_prompt():
    prompt = list(range(10))                                        # 320 rows
    cache = _cache([prompt + [20], prompt + [21]], [325, 325])
    assert cache.shared_groups([0, 1]) == ([(0, 1)], [320])
    assert cache.shared_groups([1, 0]) == ([(0, 1)], [320])          # batch indices, in batch order
    # members are batch indices of the step, whatever the ids
    cache.pages[7], cache.host_low[7] = [40, 41], 50
    assert cache.shared_groups([7, 1, 0]) == ([(1, 2)], [320])


def test_planner_common_pages_shrink_after_a_copy():
    # the prompt ended inside page 9; one fork copied it (copy on write) before it wrote there
    a, b = list(range(10)), list(range(9)) + [30]
    cache = _cache([a, b], [300, 301])
    assert cache.shared_groups([0, 1]) == ([(0, 1)], [9 * P])
    # a list that is a prefix of the other: the common pages are the shorter list
    cache = _cache([list(range(9)), list(range(12))], [288, 380])
    assert cache.shared_groups([0, 1]) == ([(0, 1)], [288])


def test_planner_eleven_forks_give_groups_of_eight_and_three():
    prompt = list(range(12))
    cache = _cache([prompt + [20 + q] for q in range(11)], [390] * 11)
    groups, rows = cache.shared_groups(list(range(11)))
    assert groups == [tuple(range(8)), (8, 9, 10)] and rows == [384, 384]
    # nine forks: the ninth would be alone in its group and is left to the one-row pass
    groups, rows = cache.shared_groups(list(range(9)))
    assert groups == [tuple(range(8))] and rows == [384]


def test_planner_cut_by_host_low_and_the_chunk_threshold():
    prompt = list(range(12))                                        # 384 rows of common pages
    cache = _cache([prompt, prompt, prompt], [384, 300, 384])
    assert cache.shared_groups([0, 1, 2]) == ([(0, 1, 2)], [300])    # the exact lower bound of the shortest member
    assert cache.shared_groups([0, 2]) == ([(0, 1)], [384])          # batch indices of the step
    cache.host_low[1] = 255
    assert cache.shared_groups([0, 1, 2]) == ([], [])                # below one 256-key chunk: no group
    cache.host_low[1] = 256
    assert cache.shared_groups([0, 1, 2]) == ([(0, 1, 2)], [256])
    short = _cache([list(range(7)) + [20], list(range(7)) + [21]], [250, 250])      # 224 shared rows
    assert short.shared_groups([0, 1]) == ([], [])
    assert kv_cache.SHARED_MIN_ROWS == 256


def test_planner_unrelated_sequences():
    cache = _cache([list(range(0, 10)), list(range(10, 20)), list(range(20, 30)), []], [320, 320, 320, 0])
    assert cache.shared_groups([0, 1, 2, 3]) == ([], [])
    # two prompts, two forks each, interleaved in the batch
    cache = _cache([list(range(0, 10)), list(range(10, 20)), list(range(0, 10)), list(range(10, 20))], [320] * 4)
    assert cache.shared_groups([0, 1, 2, 3]) == ([(0, 2), (1, 3)], [320, 320])


def test_the_plan_is_kept_until_a_page_list_changes():
    prompt = list(range(10))
    cache = _cache([prompt + [20], prompt + [21]], [325, 325], shared_decode=True)
    first = cache._step_plan([0, 1], "cpu")
    assert first.groups == [(0, 1)] and first.shared_rows == [320] and first.members.tolist()[0][:3] == [0, 1, -1]
    cache.host_low[0] = cache.host_low[1] = 340                      # rows were appended inside the last page
    assert cache._step_plan([0, 1], "cpu") is first
    cache.pages[0].append(22)                                        # sequence 0 crossed a page boundary
    second = cache._step_plan([0, 1], "cpu")
    assert second is not first and second.groups == [(0, 1)] and second.shared_rows == [320]
    assert cache._step_plan([0, 1], "cpu") is second
    assert cache._step_plan([1, 0], "cpu") is not second             # other sequences, or another order
    third = cache._step_plan([0, 1], "cpu")
    cache.pages[1][9] = 23                                           # a copy on write of a common page
    assert cache._step_plan([0, 1], "cpu") is not third
    assert cache._step_plan([0, 1], "cpu").shared_rows == [288]


# ----------------------------------------------------------------- dispatch ---
def test_the_flag_defaults_to_false():
    import inspect
    assert kv_cache.KVCache().shared_decode is False and kv_cache.KVCache().shared_plan is None
    assert kv_cache.RaggedKVCache().shared_decode is False
    assert kv_cache.PagedKVCache(4, 32).shared_decode is False
    assert kv_cache.PagedKVCache(4, 32, kv_dtype="fp8_e4m3").shared_decode is False
    assert kv_cache.PagedKVCache(4, 32, shared_decode=True).shared_decode is True
    assert kv_cache.PagedKVCache(4, 32, shared_decode=True).rows_decode is False
    assert inspect.signature(kv_cache.generate_paged).parameters["shared_decode"].default is False
    assert inspect.signature(kv_cache.PagedKVCache.__init__).parameters["shared_decode"].default is False


class _Model:
    block_size = 1024


LAYERS, HN, NT, HS, DV = 3, 2, 2, 64, 128


@pytest.fixture
def run(monkeypatch):
    """``decode_paged`` / ``append_paged`` on a real ``PagedKVCache`` with the model step stubbed: every
    layer asks the cache for its op (``decode_rows`` once per row, as ``_seq_attention_step`` and
    ``_decode_per_row`` do), and the ops record instead of launching."""
    calls = []

    def step(model, idx, cache, tbl, pos, counts, gather=None, one_row=False):
        B, Tn = idx.shape
        kv = (torch.zeros(1, P, HN, NT, HS), torch.zeros(1, P, HN, DV))
        for _ in range(LAYERS if pos is not None else 0):            # the prefill reads nothing back
            for _ in range(Tn):
                cache.decode_rows(kv, torch.zeros(B, HN, NT, HS), torch.ones(HN, NT), tbl, pos + 1)
        calls.append(("step", cache.shared_plan))
        return torch.zeros(B, Tn, 3) if gather is None else torch.zeros(B, 3)

    def record(name):
        def op(q, *a, **k):
            calls.append((name, [x for x in a if isinstance(x, ops.SharedDecodePlan)]))
            return torch.zeros(q.shape[0], HN * DV)
        return op

    monkeypatch.setattr(kv_cache, "_paged_model_step", step)
    monkeypatch.setattr(ops, "decode_shared_supported", lambda dtype, hs, N, dv, fp8=False: (hs, N, dv) == (HS, NT, DV))
    for name in ("diff_attention_decode_paged", "diff_attention_decode_paged_fp8", "diff_attention_decode_paged_shared",
                 "diff_attention_decode_paged_shared_fp8"):
        monkeypatch.setattr(ops, name, record(name.replace("diff_attention_decode_", "")))

    def make(**kw):
        cache = kv_cache.PagedKVCache(64, P, **kw)
        (root,), _ = kv_cache.prefill_paged(_Model(), [torch.zeros(300, dtype=torch.long)], cache)
        seqs = [root, cache.fork(root), cache.fork(root)]
        calls.clear()
        return cache, seqs
    make.calls = calls
    return make


def test_decode_paged_with_the_flag_reaches_the_shared_op_once_per_layer(run):
    for kw, name in ((dict(), "paged_shared"), (dict(kv_dtype="fp8_e4m3"), "paged_shared_fp8")):
        cache, seqs = run(shared_decode=True, **kw)
        kv_cache.decode_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), cache)
        ops_called = [c for c in run.calls if c[0] != "step"]
        assert [c[0] for c in ops_called] == [name] * LAYERS
        plans = [c[1][0] for c in ops_called]
        assert all(p is plans[0] for p in plans)                     # one plan, uploaded once, for every layer
        assert plans[0].groups == [(0, 1, 2)] and plans[0].shared_rows == [288]      # 9 full pages of the 300-row prompt
        assert run.calls[-1] == ("step", plans[0])
        assert cache.shared_plan is None                             # cleared when the step returns
        # a second step inside the same pages keeps the plan
        kv_cache.decode_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), cache)
        assert run.calls[-1][1] is plans[0]


def test_without_the_flag_or_a_group_the_paged_op_runs(run):
    cache, seqs = run()
    kv_cache.decode_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), cache)
    assert [c[0] for c in run.calls] == ["paged"] * LAYERS + ["step"] and run.calls[-1][1] is None
    cache, seqs = run(shared_decode=True)
    kv_cache.decode_paged(_Model(), seqs[:1], torch.zeros(1, 1, dtype=torch.long), cache)     # one sequence: no group
    assert [c[0] for c in run.calls] == ["paged"] * LAYERS + ["step"]
    assert run.calls[-1][1] is not None and run.calls[-1][1].n_groups == 0


def test_append_paged_never_reaches_the_shared_op(run):
    cache, seqs = run(shared_decode=True)
    kv_cache.append_paged(_Model(), seqs, torch.zeros(3, 2, dtype=torch.long), [2, 2, 2], cache)
    assert [c[0] for c in run.calls] == ["paged"] * (2 * LAYERS) + ["step"] and run.calls[-1][1] is None
    run.calls.clear()
    kv_cache.append_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), [1, 1, 1], cache)
    assert [c[0] for c in run.calls] == ["paged"] * LAYERS + ["step"]


def test_the_plan_is_cleared_when_the_step_raises(run, monkeypatch):
    cache, seqs = run(shared_decode=True)

    def boom(*a, **k):
        assert cache.shared_plan is not None
        raise RuntimeError("step failed")
    monkeypatch.setattr(kv_cache, "_paged_model_step", boom)
    with pytest.raises(RuntimeError, match="step failed"):
        kv_cache.decode_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), cache)
    assert cache.shared_plan is None


def test_a_shape_without_a_plan_keeps_the_paged_op(run, monkeypatch):
    monkeypatch.setattr(ops, "decode_shared_supported", lambda *a, **k: False)
    cache, seqs = run(shared_decode=True)
    kv_cache.decode_paged(_Model(), seqs, torch.zeros(3, 1, dtype=torch.long), cache)
    assert [c[0] for c in run.calls] == ["paged"] * LAYERS + ["step"]
