"""CPU checks of the graph-replayed ragged / paged step and the fused row write: ``dta_kv_step_rows``
is in the header and in the built library inside ABI 9, ``_lib.KvStepRowsArgs`` lays its struct out as
include/diffattn.h does (the gcc probe of test_fp8_cache_cpu.py), the entry point rejects bad
arguments wherever it returns before a launch, the caches validate their ``graph`` / ``fused_step``
flags, and -- with the model step and the graph stubbed, so nothing runs on a device -- a graph-mode
cache keeps the storage of ``lengths`` through ``set_lengths``, ``truncate``, ``append_ragged`` and the
decode steps, keeps one graph per (B, mask given or not), and a ``graph=False`` cache behaves as before."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_step_args_match_the_header():
    cname, py = "dta_kv_step_rows_args", _lib.KvStepRowsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    # sizeof of a call is not evaluated: nothing links, an undeclared or differently typed function does not compile
    lines += [f'  printf("symbols declared %zu\\n", sizeof(dta_kv_step_rows((const {cname}*)0, (void*)0)) / sizeof(int));',
              '  printf("abi version %d\\n", DTA_ABI_VERSION);',
              '  printf("dest kinds %d\\n", DTA_KV_STEP_CONTIGUOUS * 100 + DTA_KV_STEP_PAGED * 10 + DTA_KV_STEP_SLOTS);',
              "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
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
    assert got[("dest", "kinds")] == _lib.KV_STEP_CONTIGUOUS * 100 + _lib.KV_STEP_PAGED * 10 + _lib.KV_STEP_SLOTS == 12
    assert got[(cname, "sizeof")] == ctypes.sizeof(py)
    bad = [(f[0], got[(cname, f[0])], getattr(py, f[0]).offset) for f in py._fields_
           if got[(cname, f[0])] != getattr(py, f[0]).offset]
    assert not bad, bad


def _step_args(**kw):
    """A call that passes every host check at B = 0: no pointer is dereferenced, nothing is launched."""
    a = _lib.KvStepRowsArgs()
    a.dtype, a.B, a.Tn, a.H, a.n_terms, a.head_size, a.dv = _lib.DTA_BF16, 0, 3, 2, 2, 40, 80
    a.t_cap, a.dest = 100, _lib.KV_STEP_CONTIGUOUS
    buf = (ctypes.c_int32 * 8)()
    a.pos_dev = a.count_dev = a.block_table_dev = a.slots_out_dev = ctypes.addressof(buf)
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_step_entry_point_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.STEP_EXPORTS == ("dta_kv_step_rows",)
    for name in _lib.STEP_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert ops.kv_step_supported() is True

    class _Old:                                   # a library of the same ABI without the symbol
        dta_kv_quant_rows = None
    assert not _lib.step_symbols(_Old())

    fn = lib.dta_kv_step_rows
    paged = dict(dest=_lib.KV_STEP_PAGED, page_size=32, max_pages=4, n_pages=5)
    assert fn(None, None) == -1
    assert fn(ctypes.byref(_lib.KvStepRowsArgs()), None) == -1
    assert fn(ctypes.byref(_step_args()), None) == 0                                   # B = 0: valid, no launch
    assert fn(ctypes.byref(_step_args(Tn=0, B=2)), None) == 0
    assert fn(ctypes.byref(_step_args(**paged)), None) == 0
    assert fn(ctypes.byref(_step_args(**dict(paged, dest=_lib.KV_STEP_SLOTS))), None) == 0
    assert fn(ctypes.byref(_step_args(n_terms=8, head_size=128, dv=256)), None) == 0
    for bad in (dict(head_size=12), dict(head_size=136), dict(dv=84), dict(dv=264), dict(n_terms=9)):
        assert fn(ctypes.byref(_step_args(**bad)), None) == -2, bad
    here = _step_args().pos_dev
    for bad in (dict(dtype=3), dict(n_terms=0), dict(B=-1), dict(dest=3), dict(dest=-1), dict(t_cap=0),
                dict(t_cap=2 ** 30 + 1), dict(pos_dev=None), dict(pos_dev=here + 2), dict(count_dev=None),
                dict(count_dev=here + 1), dict(paged, page_size=48), dict(paged, n_pages=0), dict(paged, max_pages=0),
                dict(paged, max_pages=3),                     # 3 pages of 32 rows do not reach t_cap 100
                dict(paged, block_table_dev=None), dict(paged, block_table_dev=here + 2),
                dict(paged, dest=_lib.KV_STEP_SLOTS, slots_out_dev=None),
                dict(paged, dest=_lib.KV_STEP_SLOTS, slots_out_dev=here + 2)):
        assert fn(ctypes.byref(_step_args(**bad)), None) == -1, bad
    # B > 0: a misaligned view is refused before any launch (the pointers are never read on the host)
    mis = _step_args(B=1)
    for t in (mis.q, mis.k, mis.v, mis.q_out, mis.k_dst, mis.v_dst):
        t.ptr, t.sb, t.st, t.sh, t.si = 4096, 4096, 1024, 160, 40
    mis.v.sh = 84                                 # 84 elements: not a multiple of 16 bytes
    assert fn(ctypes.byref(mis), None) == -1


def test_flag_validation(monkeypatch):
    for make in (lambda **kw: kv_cache.RaggedKVCache(**kw), lambda **kw: kv_cache.PagedKVCache(4, 32, **kw)):
        c = make()
        assert c.use_graph is False and c.fused_step is False and c.graphs == {}
        c = make(graph=True, fused_step=True)
        assert c.use_graph is True and c.fused_step is True
    assert kv_cache.KVCache().fused_step is False
    with pytest.raises(ValueError, match="shared_decode"):
        kv_cache.PagedKVCache(4, 32, graph=True, shared_decode=True)
    kv_cache.PagedKVCache(4, 32, fused_step=True, shared_decode=True)        # the fused write alone is fine
    monkeypatch.setattr(ops, "kv_step_supported", lambda: False)            # a library without the symbol
    with pytest.raises(RuntimeError, match="dta_kv_step_rows"):
        kv_cache.RaggedKVCache(fused_step=True)
    with pytest.raises(RuntimeError, match="dta_kv_step_rows"):
        kv_cache.PagedKVCache(4, 32, fused_step=True)
    kv_cache.RaggedKVCache(graph=True)                                       # the graph alone needs no new symbol


class _Model:
    block_size = 64


class _FakeGraph:
    """What ``SeqDecodeGraph`` does to the cache, without a device: the length update, in place."""
    made = []

    def __init__(self, model, cache, B, device, slots=None):
        self.cache, self.B, self.paged = cache, B, slots is not None
        self.steps = 0
        _FakeGraph.made.append(self)

    def step(self, tok, counts, slots=None):
        self.steps += 1
        if self.paged:
            self.cache.lengths.index_copy_(0, slots, self.cache.lengths.index_select(0, slots) + counts)
        else:
            self.cache.lengths.add_(counts)
        return torch.zeros(self.B, 3)


@pytest.fixture
def stubbed(monkeypatch):
    def ragged(model, idx, cache, pos, counts, gather=None, one_row=False):
        return torch.zeros(idx.shape[0], 3) if gather is not None else torch.zeros(idx.shape[0], idx.shape[1], 3)

    def paged(model, idx, cache, tbl, pos, counts, gather=None, one_row=False):
        return ragged(model, idx, cache, pos, counts, gather, one_row)

    _FakeGraph.made = []
    monkeypatch.setattr(kv_cache, "_ragged_model_step", ragged)
    monkeypatch.setattr(kv_cache, "_paged_model_step", paged)
    monkeypatch.setattr(kv_cache, "SeqDecodeGraph", _FakeGraph)
    return _FakeGraph


def _prompts(*lens):
    return [torch.arange(n, dtype=torch.long) % 5 for n in lens]


def test_graph_mode_keeps_the_lengths_storage(stubbed):
    model = _Model()
    cache = kv_cache.RaggedKVCache(graph=True)
    kv_cache.prefill_ragged(model, _prompts(5, 9, 2), cache)
    held = cache.lengths
    tok = torch.zeros(3, 1, dtype=torch.long)
    kv_cache.decode_ragged(model, tok, cache)
    kv_cache.decode_ragged(model, tok, cache)
    assert cache.lengths is held and held.tolist() == [7, 11, 4] and cache.host_lengths == [7, 11, 4]
    assert list(cache.graphs) == [(3, False)] and stubbed.made[0].steps == 2
    kv_cache.decode_ragged(model, tok, cache, active=torch.tensor([True, False, True]))
    assert cache.lengths is held and held.tolist() == [8, 11, 5]
    assert sorted(cache.graphs) == [(3, False), (3, True)] and len(stubbed.made) == 2     # one per (B, mask given)
    assert cache.host_exact is False and cache.sync() == [8, 11, 5] and cache.lengths is held
    cache.truncate([6, 11, 0])
    assert cache.lengths is held and held.tolist() == [6, 11, 0] and cache.host_lengths == [6, 11, 0]
    cache.set_lengths([1, 2, 3], "cpu")
    assert cache.lengths is held and held.tolist() == [1, 2, 3]
    kv_cache.append_ragged(model, torch.zeros(3, 4, dtype=torch.long), [4, 0, 2], cache)     # eager, but in place
    assert cache.lengths is held and held.tolist() == [5, 2, 5] and len(cache.graphs) == 2
    # another batch size: the rows are reallocated with it, so the graphs go and the lengths are new
    kv_cache.prefill_ragged(model, _prompts(4, 4), cache)
    assert cache.lengths is not held and cache.lengths.tolist() == [4, 4] and cache.graphs == {}


def test_without_graph_the_ragged_cache_rebinds_as_before(stubbed):
    model = _Model()
    cache = kv_cache.RaggedKVCache()
    kv_cache.prefill_ragged(model, _prompts(5, 9, 2), cache)
    held = cache.lengths
    kv_cache.decode_ragged(model, torch.zeros(3, 1, dtype=torch.long), cache)
    assert cache.lengths is not held and held.tolist() == [5, 9, 2] and cache.lengths.tolist() == [6, 10, 3]
    held = cache.lengths
    cache.truncate([6, 1, 3])
    assert cache.lengths is not held and held.tolist() == [6, 10, 3] and cache.lengths.tolist() == [6, 1, 3]
    held = cache.lengths
    kv_cache.append_ragged(model, torch.zeros(3, 2, dtype=torch.long), [1, 2, 0], cache)
    assert cache.lengths is not held and cache.lengths.tolist() == [7, 3, 3]
    assert cache.graphs == {} and not stubbed.made


def test_paged_graph_mode_bookkeeping(stubbed):
    """The host side of a graph-mode ``decode_paged``: pages grow and tables are flushed before the replay,
    the graph gets the step's slots, a subset of another size gets a graph of its own."""
    model = _Model()
    cache = kv_cache.PagedKVCache(8, 32, graph=True)
    (a, b, c), _ = kv_cache.prefill_paged(model, _prompts(31, 32, 5), cache)
    held = cache.lengths
    tok = torch.zeros(3, 1, dtype=torch.long)
    kv_cache.decode_paged(model, [a, b, c], tok, cache)
    kv_cache.decode_paged(model, [c, a, b], tok, cache)                      # another order: the same graph
    assert cache.lengths is held and cache.sync() == {a: 33, b: 34, c: 7}
    assert [held[cache.slot[q]].item() for q in (a, b, c)] == [33, 34, 7]
    assert len(cache.pages[a]) == 2 and len(cache.pages[b]) == 2 and len(cache.pages[c]) == 1
    assert cache.block_table[cache.slot[a]].tolist()[:2] == cache.pages[a]   # flushed before the replay
    assert list(cache.graphs) == [(3, False)] and stubbed.made[0].steps == 2
    kv_cache.decode_paged(model, [b], tok[:1], cache)
    kv_cache.decode_paged(model, [c, a], tok[:2], cache, active=torch.tensor([False, True]))
    assert sorted(cache.graphs) == [(1, False), (2, True), (3, False)]
    assert cache.sync() == {a: 34, b: 35, c: 7} and cache.lengths is held
    cache.truncate(b, 3)
    kv_cache.decode_paged(model, [a, b, c], tok, cache)
    assert cache.sync() == {a: 35, b: 4, c: 8} and stubbed.made[0].steps == 3


def test_a_graph_needs_a_prefilled_cache():
    with pytest.raises(ValueError, match="prefilled"):
        kv_cache.SeqDecodeGraph(_Model(), kv_cache.RaggedKVCache(graph=True), 2, "cpu")
    cache = kv_cache.PagedKVCache(4, 32, graph=True)
    with pytest.raises(ValueError, match="prefilled"):
        kv_cache.SeqDecodeGraph(_Model(), cache, 2, "cpu", slots=torch.zeros(2, dtype=torch.long))
