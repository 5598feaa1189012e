"""CPU checks of the paged KV cache: ``_lib.DecodePagedArgs`` / ``ExtendPagedArgs`` lay out
``dta_attn_decode_paged_args`` / ``dta_attn_extend_paged_args`` exactly as include/diffattn.h
does (the gcc sizeof / offsetof probe of test_abi_layout.py), the built library exports
both entry points, still reports ABI 9 and rejects bad page arguments without a device,
and the host allocator of ``kv_cache.PagedKVCache`` (free list, refcounts, page lists,
copy on write, out-of-pages) with the model step stubbed, so no kernel runs."""
import copy
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "dta_attn_decode_paged_args": _lib.DecodePagedArgs,
    "dta_attn_extend_paged_args": _lib.ExtendPagedArgs,
}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_paged_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ['  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    assert got[("abi", "version")] == _lib.ABI_VERSION == 9         # the feature arrives without an ABI bump
    bad = []
    for cname, py in STRUCTS.items():
        if got[(cname, "sizeof")] != ctypes.sizeof(py):
            bad.append((cname, "sizeof", got[(cname, "sizeof")], ctypes.sizeof(py)))
        for f in py._fields_:
            off = getattr(py, f[0]).offset
            if got[(cname, f[0])] != off:
                bad.append((cname, f[0], got[(cname, f[0])], off))
    assert not bad, bad
    # the paged structs are the ragged ones with the cache views renamed and four fields appended
    rename = {"k_cache": "k_pool", "v_cache": "v_pool"}
    tail = ["page_size", "max_pages", "n_pages", "block_table_dev"]
    for ragged, paged in ((_lib.DecodeRaggedArgs, _lib.DecodePagedArgs), (_lib.ExtendRaggedArgs, _lib.ExtendPagedArgs)):
        assert [rename.get(f[0], f[0]) for f in ragged._fields_] + tail == [f[0] for f in paged._fields_]


def _decode_args(**kw):
    """A paged decode call that passes every host check that precedes the page checks
    (dims, length <= t_cap) at B = 0, so no pointer is looked at and nothing is launched."""
    a = _lib.DecodePagedArgs()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_F32, 0, 2, 2, 64, 128
    a.length, a.t_cap, a.scale = 8, 128, 0.125
    a.page_size, a.max_pages, a.n_pages = 64, 2, 4
    buf = (ctypes.c_int32 * 4)()
    a.lengths_dev = ctypes.addressof(buf)
    a.block_table_dev = ctypes.addressof(buf)
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _extend_args(**kw):
    a = _lib.ExtendPagedArgs()
    a.dtype, a.B, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_F32, 0, 2, 2, 64, 128
    a.Tq, a.t_cap, a.scale = 4, 128, 0.125
    a.page_size, a.max_pages, a.n_pages = 64, 2, 4
    buf = (ctypes.c_int32 * 4)()
    a.pos_dev = ctypes.addressof(buf)
    a.block_table_dev = ctypes.addressof(buf)
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_paged_entry_points():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    for name in ("dta_attn_decode_paged", "dta_attn_extend_paged"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # argument validation needs no device
    assert lib.dta_attn_decode_paged(None, None) == -1
    assert lib.dta_attn_extend_paged(None, None) == -1
    assert lib.dta_attn_decode_paged(ctypes.byref(_lib.DecodePagedArgs()), None) == -1
    assert lib.dta_attn_extend_paged(ctypes.byref(_lib.ExtendPagedArgs()), None) == -1
    for make, fn in ((_decode_args, lib.dta_attn_decode_paged), (_extend_args, lib.dta_attn_extend_paged)):
        assert fn(ctypes.byref(make()), None) == 0                               # B = 0: valid, no launch
        assert fn(ctypes.byref(make(page_size=32, max_pages=4)), None) == 0
        assert fn(ctypes.byref(make(page_size=256, max_pages=1, t_cap=256)), None) == 0
        assert fn(ctypes.byref(make(page_size=48, max_pages=2, t_cap=96)), None) == -1
        assert fn(ctypes.byref(make(page_size=512, max_pages=1, t_cap=512)), None) == -1
        assert fn(ctypes.byref(make(t_cap=127)), None) == -1                     # t_cap != max_pages * page_size
        assert fn(ctypes.byref(make(max_pages=3)), None) == -1
        assert fn(ctypes.byref(make(block_table_dev=None)), None) == -1          # null table
        assert fn(ctypes.byref(make(block_table_dev=make().block_table_dev + 2)), None) == -1   # misaligned table
        assert fn(ctypes.byref(make(n_pages=0)), None) == -1


# --------------------------------------------------------------- allocator ---
class _Model:
    block_size = 256


P, POOL = 32, 12


@pytest.fixture
def calls(monkeypatch):
    out = []

    def step(model, idx, cache, tbl, pos, counts, gather=None, one_row=False):
        out.append((tuple(idx.shape), tbl.tolist(), None if pos is None else pos.tolist(), counts.tolist(),
                    None if gather is None else gather.tolist(), one_row))
        if gather is None:
            return torch.zeros(idx.shape[0], idx.shape[1], 3)
        return torch.zeros(idx.shape[0], 3)

    monkeypatch.setattr(kv_cache, "_paged_model_step", step)
    return out


def _prompts(*lens):
    return [torch.arange(n, dtype=torch.long) % 5 for n in lens]


def _tok(n=1, B=1):
    return torch.zeros(B, n, dtype=torch.long)


def _snapshot(cache):
    cache._flush()
    return copy.deepcopy((cache.free, cache.refcount, cache.pages, cache.host_lengths, cache.slot,
                          cache.block_table.tolist(), cache.lengths.tolist()))


def _consistent(cache):
    """Every page is free or referenced, and the refcounts are the page lists' counts."""
    count = [0] * cache.num_pages
    for pages in cache.pages.values():
        for pg in pages:
            count[pg] += 1
    assert count == cache.refcount
    assert sorted(cache.free) == [pg for pg in range(cache.num_pages) if count[pg] == 0]
    cache._flush()
    for q, sl in cache.slot.items():
        row = cache.block_table[sl].tolist()
        assert row == cache.pages[q] + [-1] * (cache.max_pages - len(cache.pages[q]))


def _row(pages, max_pages=8):
    return pages + [-1] * (max_pages - len(pages))


def test_prefill_takes_pages_and_decode_crosses_a_boundary(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), logits = kv_cache.prefill_paged(model, _prompts(40, 100), cache)
    assert logits.shape == (2, 3)
    assert cache.max_pages == 8 and cache.block_table.shape == (POOL, 8) and cache.block_table.dtype == torch.int32
    assert len(cache.pages[a]) == 2 and len(cache.pages[b]) == 4 and cache.pages_in_use() == 6
    assert calls == [((2, 100), [_row(cache.pages[a]), _row(cache.pages[b])], None, [40, 100], [39, 99], False)]
    assert cache.host_lengths == {a: 40, b: 100}
    _consistent(cache)

    # 24 decode steps take A from 40 to 64: rows 40 .. 63 fit its second page
    for n in range(24):
        kv_cache.decode_paged(model, [a], _tok(), cache)
    assert cache.pages_in_use() == 6 and cache.host_lengths[a] == 64
    # the next row is the first of a new page: exactly one page is taken
    kv_cache.decode_paged(model, [a], _tok(), cache)
    assert cache.pages_in_use() == 7 and len(cache.pages[a]) == 3 and cache.host_lengths[a] == 65
    assert calls[-1] == ((1, 1), [_row(cache.pages[a])], [64], [1], None, True)
    assert cache.lengths[cache.slot[a]].item() == 65 and cache.lengths[cache.slot[b]].item() == 100
    kv_cache.decode_paged(model, [b, a], _tok(B=2), cache)                      # any subset, any order
    assert calls[-1][2] == [100, 65] and cache.pages_in_use() == 7
    _consistent(cache)


def test_release_returns_pages_and_prefill_reuses_them(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), _ = kv_cache.prefill_paged(model, _prompts(40, 100), cache)
    a_pages = list(cache.pages[a])
    cache.release(a)
    assert cache.pages_in_use() == 4 and a not in cache.pages and all(cache.refcount[pg] == 0 for pg in a_pages)
    (c,), _ = kv_cache.prefill_paged(model, _prompts(70), cache)                # into the live cache
    assert c not in (a, b)                                                      # ids are never reused
    assert len(cache.pages[c]) == 3 and set(a_pages) <= set(cache.pages[c])
    _consistent(cache)
    with pytest.raises(ValueError):
        cache.release(a)                                                        # a double release
    with pytest.raises(ValueError):
        kv_cache.decode_paged(model, [a], _tok(), cache)                        # a step naming a released sequence
    with pytest.raises(ValueError):
        kv_cache.append_paged(model, [b, a], _tok(2, 2), [1, 1], cache)
    with pytest.raises(ValueError):
        kv_cache.decode_paged(model, [b, b], _tok(B=2), cache)                  # named twice
    with pytest.raises(ValueError):
        cache.fork(a)
    _consistent(cache)


def test_truncate_frees_whole_pages_only(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), _ = kv_cache.prefill_paged(model, _prompts(40, 100), cache)
    pages = list(cache.pages[b])
    cache.truncate(b, 97)                                                       # still four pages
    assert cache.pages[b] == pages and cache.host_lengths[b] == 97
    cache.truncate(b, 96)                                                       # exactly three
    assert cache.pages[b] == pages[:3] and cache.refcount[pages[3]] == 0 and pages[3] in cache.free
    cache.truncate(b, 33)
    assert cache.pages[b] == pages[:2] and cache.pages_in_use() == 4
    for bad in (34, -1):
        with pytest.raises(ValueError):
            cache.truncate(b, bad)
    cache.truncate(b, 0)
    assert cache.pages[b] == [] and cache.pages_in_use() == 2
    _consistent(cache)
    kv_cache.decode_paged(model, [b], _tok(), cache)                            # an empty sequence grows again
    assert calls[-1][2] == [0] and len(cache.pages[b]) == 1 and cache.lengths[cache.slot[b]].item() == 1
    _consistent(cache)


def test_fork_shares_and_the_first_write_copies_the_partial_page(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a,), _ = kv_cache.prefill_paged(model, _prompts(70), cache)                # two full pages and 6 rows
    pages = list(cache.pages[a])
    before = cache.pages_in_use()
    c = cache.fork(a)
    d = cache.fork(a)
    assert cache.pages_in_use() == before == 3                                  # no page added
    assert cache.pages[c] == pages and cache.pages[d] == pages and cache.pages[c] is not cache.pages[a]
    assert [cache.refcount[pg] for pg in pages] == [3, 3, 3]
    assert cache.host_lengths[c] == cache.host_lengths[d] == 70
    _consistent(cache)
    # the first write of C copies the partial page, and never a full shared one
    kv_cache.decode_paged(model, [c], _tok(), cache)
    assert cache.pages[c][:2] == pages[:2] and cache.pages[c][2] not in pages
    assert [cache.refcount[pg] for pg in pages] == [3, 3, 2] and cache.pages_in_use() == 4
    assert calls[-1][1] == [_row(cache.pages[c])]
    # A and D step together: one of them copies, the last holder keeps the page
    kv_cache.decode_paged(model, [a, d], _tok(B=2), cache)
    assert cache.pages_in_use() == 5
    assert [cache.refcount[pg] for pg in pages] == [3, 3, 1]
    assert cache.pages[a][:2] == cache.pages[d][:2] == pages[:2] and cache.pages[a][2] != cache.pages[d][2]
    # from now on nobody copies
    kv_cache.decode_paged(model, [a, c, d], _tok(B=3), cache)
    assert cache.pages_in_use() == 5
    # a fork on a page boundary shares full pages only: the first write takes a page, copies none
    (e,), _ = kv_cache.prefill_paged(model, _prompts(64), cache)
    f = cache.fork(e)
    used = cache.pages_in_use()
    kv_cache.append_paged(model, [f], _tok(3), [3], cache)
    assert cache.pages[f][:2] == cache.pages[e] and cache.pages_in_use() == used + 1
    assert [cache.refcount[pg] for pg in cache.pages[e]] == [2, 2]
    # releasing a sharer keeps the shared pages alive
    cache.release(a)
    assert [cache.refcount[pg] for pg in pages[:2]] == [2, 2]
    _consistent(cache)


def test_copy_on_write_copies_the_page_in_every_layer(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a,), _ = kv_cache.prefill_paged(model, _prompts(40), cache)
    for layer in (1, 2):
        pool = cache.layer_pool(layer, 4, torch.zeros(1))
        pool.copy_(torch.arange(pool.numel(), dtype=torch.float32).view_as(pool) + 1000 * layer)
    c = cache.fork(a)
    old = cache.pages[a][1]
    kv_cache.append_paged(model, [c], _tok(2), [2], cache)
    new = cache.pages[c][1]
    assert new != old and cache.pages[a][1] == old
    for layer in (1, 2):
        assert torch.equal(cache.pool[layer][new], cache.pool[layer][old])


def test_out_of_pages_leaves_everything_unchanged(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), _ = kv_cache.prefill_paged(model, _prompts(40, 100), cache)         # 6 pages, 6 free
    c = cache.fork(b)
    n = len(calls)
    snap = _snapshot(cache)
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.prefill_paged(model, _prompts(100, 100), cache)                # 8 > 6
    assert _snapshot(cache) == snap and len(calls) == n
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.append_paged(model, [a, c], _tok(156, 2), [156, 100], cache)   # 5 + (1 copy + 3) > 6
    assert _snapshot(cache) == snap and len(calls) == n
    kv_cache.append_paged(model, [a], _tok(152), [152], cache)                  # 40 -> 192: four more pages
    assert cache.pages_in_use() == 10 and len(calls) == n + 1
    (d,), _ = kv_cache.prefill_paged(model, _prompts(33), cache)                # the last two pages
    assert cache.free == []
    n = len(calls)
    snap = _snapshot(cache)
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.decode_paged(model, [c], _tok(), cache)                        # the fork's copy has no page to go to
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.decode_paged(model, [a, d], _tok(B=2), cache)                  # A at 192 needs a seventh page
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.prefill_paged(model, _prompts(1), cache)
    assert _snapshot(cache) == snap and len(calls) == n
    kv_cache.decode_paged(model, [d], _tok(), cache)                            # D still has room in its page
    cache.release(b)                                                            # C holds B's pages alone now
    kv_cache.decode_paged(model, [c], _tok(), cache)
    assert cache.free == [] and cache.host_lengths[c] == 101
    _consistent(cache)
    assert issubclass(kv_cache.OutOfPages, RuntimeError)


def test_active_mask_allocates_on_the_upper_bound(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), _ = kv_cache.prefill_paged(model, _prompts(64, 10), cache)
    mask = torch.tensor([False, True])
    kv_cache.decode_paged(model, [a, b], _tok(B=2), cache, active=mask)
    assert calls[-1][3] == [0, 1]
    assert not cache.host_exact and cache.host_lengths == {a: 65, b: 11}        # upper bounds
    assert len(cache.pages[a]) == 3                                             # a page for the bound
    assert cache.lengths[cache.slot[a]].item() == 64 and cache.lengths[cache.slot[b]].item() == 11
    assert cache.sync() == {a: 64, b: 11} and cache.host_exact
    assert len(cache.pages[a]) == 2 and cache.pages_in_use() == 3               # the surplus came back
    _consistent(cache)


def test_append_near_block_size_runs_narrower_steps(calls):
    model, cache = _Model(), kv_cache.PagedKVCache(POOL, P)
    (a, b), _ = kv_cache.prefill_paged(model, _prompts(254, 2), cache)
    del calls[:]
    rows = kv_cache.append_paged(model, [a, b], _tok(5, 2), [2, 5], cache, all_rows=True)
    assert rows.shape == (2, 5, 3)
    assert [(c[0], c[2], c[3]) for c in calls] == [((2, 2), [254, 2], [2, 2]), ((2, 3), [256, 4], [0, 3])]
    assert cache.host_lengths == {a: 256, b: 7}
    with pytest.raises(ValueError):
        kv_cache.decode_paged(model, [a], _tok(), cache)                        # 256 + 1 > block_size
    with pytest.raises(ValueError):
        kv_cache.append_paged(model, [a, b], _tok(2, 2), [1, 1], cache)
    with pytest.raises(ValueError):
        kv_cache.append_paged(model, [a, b], _tok(2, 2), [0, 3], cache)         # count > Tn


def test_generate_paged_bookkeeping(calls, monkeypatch):
    model = _Model()
    with pytest.raises(ValueError):
        kv_cache.generate_paged(model, _prompts(3, 250), 7)                     # 250 + 7 > block_size
    assert calls == []
    with pytest.raises(ValueError):
        kv_cache.PagedKVCache(4, 48)
    with pytest.raises(ValueError):
        kv_cache.PagedKVCache(0, 64)
    for name in ("PagedKVCache", "OutOfPages", "prefill_paged", "decode_paged", "append_paged", "generate_paged"):
        assert name in kv_cache.__all__
    # sequence 0 samples eos_id = 2 at its second token: its length is frozen from then on
    samples = iter([[1, 1], [2, 3], [4, 3], [2, 2]])
    monkeypatch.setattr(torch, "multinomial", lambda probs, num_samples: torch.tensor(next(samples))[:, None])
    out = kv_cache.generate_paged(model, _prompts(3, 7), 4, eos_id=2, page_size=32)
    assert [o.tolist() for o in out] == [[0, 1, 2, 1, 2], [0, 1, 2, 3, 4, 0, 1, 1, 3, 3, 2]]
    assert [c[2] for c in calls] == [None, [3, 7], [4, 8], [4, 9]]
    assert [c[3] for c in calls][1:] == [[1, 1], [0, 1], [0, 1]]
    # three samples of a 70-token prompt, 5 new tokens, P = 32: two shared full pages and
    # three copies of the partial one are exactly enough; one page fewer is not
    monkeypatch.setattr(torch, "multinomial", lambda probs, num_samples: torch.zeros(probs.shape[0], 1, dtype=torch.long))
    out = kv_cache.generate_paged(model, _prompts(70), 5, n_samples=3, num_pages=5, page_size=32)
    assert len(out) == 1 and [len(o) for o in out[0]] == [75, 75, 75]
    tables = calls[-1][1]
    assert tables[0][:2] == tables[1][:2] == tables[2][:2] and len({t[2] for t in tables}) == 3
    out = kv_cache.generate_paged(model, _prompts(70), 5, n_samples=3, page_size=32)        # the default is that need
    assert [len(o) for o in out[0]] == [75, 75, 75]
    with pytest.raises(kv_cache.OutOfPages):
        kv_cache.generate_paged(model, _prompts(70), 5, n_samples=3, num_pages=4, page_size=32)
