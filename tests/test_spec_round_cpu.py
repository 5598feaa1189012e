"""CPU checks of the fixed-shape speculative round: ``dta_spec_feed_rows`` / ``dta_spec_commit_lengths`` in the
header and the built library inside ABI 9 with the structs laid out as ``_lib`` says and every validation code
they return before a launch; ``ops.spec_feed_rows_reference`` / ``ops.spec_commit_lengths_reference`` against a
line-by-line reading of the definition (``_spec_round``), edge rows and out-of-range device values included; and
``Speculation(graph=True)`` on CPU tensors with the model step stubbed, where the round's body runs uncaptured
through the references: the plain sampler loop's tokens, the eager round's stats and pages, the eager fallback
next to the window's end, and nothing of it with the flag off."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

import _spec as S
import _spec_round as R
from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"dta_spec_feed_rows": _lib.SpecFeedRowsArgs, "dta_spec_commit_lengths": _lib.SpecCommitLengthsArgs}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_round_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for fn, py in STRUCTS.items():
        lines.append(f'  printf("{fn}_args sizeof %zu\\n", sizeof({fn}_args));')
        for f in py._fields_:
            lines.append(f'  printf("{fn}_args {f[0]} %zu\\n", offsetof({fn}_args, {f[0]}));')
        lines.append(f'  printf("{fn} declared %zu\\n", sizeof({fn}((const {fn}_args*)0, (void*)0)) / sizeof(int));')
    lines += ['  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
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
    assert got[("abi", "version")] == _lib.ABI_VERSION == 9
    for fn, py in STRUCTS.items():
        assert got[(fn, "declared")] == 1
        assert got[(fn + "_args", "sizeof")] == ctypes.sizeof(py)
        bad = [(f[0], got[(fn + "_args", f[0])], getattr(py, f[0]).offset) for f in py._fields_
               if got[(fn + "_args", f[0])] != getattr(py, f[0]).offset]
        assert not bad, bad


_BUF = (ctypes.c_int64 * 8)()
HERE = ctypes.addressof(_BUF)


def _feed_args(**kw):
    """A call that passes every host check at B = 0: no pointer is read, nothing is launched."""
    a = _lib.SpecFeedRowsArgs()
    a.B, a.K, a.cap, a.vocab, a.total = 0, 3, 64, 13, 12
    a.hist_stride, a.draft_stride, a.idx_stride, a.offset_stride = 64, 3, 4, 4
    a.hist = a.hlen_dev = a.remaining_dev = a.draft = a.dcnt_dev = a.idx_out = a.counts_out = a.offset_out = HERE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _commit_args(**kw):
    a = _lib.SpecCommitLengthsArgs()
    a.B, a.K, a.t_cap, a.n_slots = 0, 3, 64, 8
    a.lengths = a.result = a.slots = HERE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_kernels_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.SPEC_ROUND_EXPORTS == ("dta_spec_feed_rows", "dta_spec_commit_lengths")
    for name in _lib.SPEC_ROUND_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert ops.spec_round_supported() is True

    class _Old:
        dta_spec_accept_draft = None
        dta_spec_feed_rows = None
    assert not _lib.spec_round_symbols(_Old())

    feed = lib.dta_spec_feed_rows
    assert feed(None, None) == -1
    assert feed(ctypes.byref(_feed_args()), None) == 0                             # B = 0: valid, no launch
    for ok in (dict(K=1, draft_stride=1, idx_stride=2, offset_stride=2), dict(K=7, draft_stride=7, idx_stride=8, offset_stride=8),
               dict(vocab=1), dict(total=0), dict(hist_stride=100, idx_stride=9), dict(cap=1 << 30, hist_stride=1 << 30)):
        assert feed(ctypes.byref(_feed_args(**ok)), None) == 0, ok
    for bad in (dict(B=-1), dict(K=0), dict(K=8, draft_stride=8, idx_stride=9, offset_stride=9), dict(vocab=0), dict(total=-1),
                dict(cap=0), dict(cap=(1 << 30) + 1, hist_stride=1 << 31), dict(hist_stride=63), dict(draft_stride=2),
                dict(idx_stride=3), dict(offset_stride=3),
                dict(hist=None), dict(hlen_dev=None), dict(remaining_dev=None), dict(draft=None), dict(dcnt_dev=None),
                dict(idx_out=None), dict(counts_out=None), dict(offset_out=None),
                dict(hist=HERE + 2), dict(hlen_dev=HERE + 1), dict(remaining_dev=HERE + 2), dict(draft=HERE + 2),
                dict(dcnt_dev=HERE + 3), dict(idx_out=HERE + 4), dict(counts_out=HERE + 2), dict(offset_out=HERE + 4)):
        assert feed(ctypes.byref(_feed_args(**bad)), None) == -1, bad

    commit = lib.dta_spec_commit_lengths
    assert commit(None, None) == -1
    assert commit(ctypes.byref(_commit_args()), None) == 0
    for ok in (dict(K=1), dict(K=7), dict(slots=None), dict(n_slots=1), dict(t_cap=1 << 30)):
        assert commit(ctypes.byref(_commit_args(**ok)), None) == 0, ok
    for bad in (dict(B=-1), dict(K=0), dict(K=8), dict(t_cap=0), dict(t_cap=(1 << 30) + 1), dict(n_slots=0),
                dict(B=9, slots=None), dict(lengths=None), dict(result=None),
                dict(lengths=HERE + 2), dict(result=HERE + 1), dict(slots=HERE + 4)):
        assert commit(ctypes.byref(_commit_args(**bad)), None) == -1, bad


# ------------------------------------------------------------------ the references ---
@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("B", R.BATCHES)
def test_feed_reference_is_the_definition(B, K):
    seen = set()
    for tag, st in R.states(B, K):
        before = st.clone()
        idx, counts, offset = ops.spec_feed_rows_reference(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K,
                                                           R.VOCAB, R.TOTAL)
        assert (idx.dtype, counts.dtype, offset.dtype) == (torch.int64, torch.int32, torch.int64)
        assert idx.shape == offset.shape == (B, K + 1) and counts.shape == (B,)
        R.check_feed(st, K, idx, counts, offset)
        for new, old in zip(st.tensors(), before.tensors()):                       # the state is read only
            assert torch.equal(new, old), tag
        assert ops.spec_feed_rows(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K, R.VOCAB, R.TOTAL)[0].equal(idx)
        seen |= set(counts.tolist())
    assert seen >= {0, 1, K + 1}
    # given outputs, a padded row stride included: every entry is written
    st = S.random_state(B, R.HLENS, R.CAP, R.VOCAB, K, seed=5)
    wide = torch.full((2, B, K + 4), -7, dtype=torch.int64)
    counts = torch.full((B,), -7, dtype=torch.int32)
    out = ops.spec_feed_rows(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K, R.VOCAB, R.TOTAL,
                             wide[0, :, 2:K + 3], counts, wide[1, :, 2:K + 3])
    assert out[0].data_ptr() == wide[0, :, 2:].data_ptr() and out[1] is counts
    R.check_feed(st, K, *out)
    assert int((wide == -7).sum()) == 2 * B * 3


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("B", R.BATCHES)
def test_commit_reference_is_the_definition(B, K, paged):
    lengths, result, slots = R.commit_inputs(B, K, 64, paged)
    want = R.definition_commit(lengths.tolist(), result.tolist(), K, 64, None if slots is None else slots.tolist())
    res0, slots0 = result.clone(), None if slots is None else slots.clone()
    got = ops.spec_commit_lengths_reference(lengths.clone(), result, K, 64, slots)
    assert got.dtype == torch.int32 and got.tolist() == want
    assert max(want) <= 64 and (B == 1 or want != lengths.tolist())
    assert torch.equal(result, res0) and (slots is None or torch.equal(slots, slots0))
    mine = lengths.clone()
    assert ops.spec_commit_lengths(mine, result, K, 64, slots) is mine and mine.tolist() == want
    if paged:                                   # the slots nobody names are as they were
        named = set(slots.clamp(0, B + 4).tolist())
        assert all(want[s] == int(lengths[s]) for s in range(B + 5) if s not in named) and len(named) == B


def test_wrappers_reject_bad_arguments():
    st = S.random_state(2, [5], 16, 3, 3, seed=1)
    feed = lambda **kw: ops.spec_feed_rows(*[kw.get(n, getattr(st, n)) for n in ("hist", "hlen", "remaining", "draft", "dcnt")],  # noqa: E731
                                           kw.get("k", 3), kw.get("vocab", 3), kw.get("total", 8), kw.get("idx_out"))
    for kw in (dict(k=0), dict(k=8), dict(vocab=0), dict(total=-1), dict(hist=st.hist.long()), dict(hlen=st.hlen[:1]),
               dict(draft=st.draft[:, :2]), dict(idx_out=torch.zeros(2, 4, dtype=torch.int32)),
               dict(idx_out=torch.zeros(2, 8, dtype=torch.int64)[:, ::2])):
        with pytest.raises(ValueError):
            feed(**kw)
    lengths, result = S.i32([3, 4]), S.i32([[1, 0], [2, 0]])
    for a in ((lengths.long(), result, 3, 64), (lengths, result.long(), 3, 64), (lengths, result, 0, 64), (lengths, result, 3, 0),
              (lengths[:1], result, 3, 64), (lengths, result, 3, 64, torch.tensor([0, 1], dtype=torch.int32)),
              (lengths, result, 3, 64, torch.tensor([0]))):
        with pytest.raises(ValueError):
            ops.spec_commit_lengths(*a)


# ------------------------------------------------------------------ the loops ---
def _generate(kind, model, prompts, n, monkeypatch, **kw):
    """(outputs, the paged call's cache or None)."""
    if kind == "ragged":
        return kv_cache.generate_ragged(model, prompts, n, **kw), None
    monkeypatch.setattr(kv_cache, "PagedKVCache", S.RecordingPagedCache)
    out = kv_cache.generate_paged(model, prompts, n, page_size=32, **kw)
    return out, S.RecordingPagedCache.last


def test_speculation_graph_flag():
    assert kv_cache.Speculation().graph is False
    s = kv_cache.Speculation(k=2, graph=True)
    assert s.graph is True and "graph=True" in repr(s) and "graph" not in repr(kv_cache.Speculation(k=2))
    with pytest.raises(AttributeError):
        s.graph = False


@pytest.mark.parametrize("eos", [None, 4])
@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_fixed_shape_round_is_the_plain_loop(kind, eos, monkeypatch):
    S.stub_steps(monkeypatch)
    model, k, n = S.Model(), 3, 10
    prompts = S.prompts(28, 31, 5)              # paged, 32-row pages: rounds cross a page boundary
    smp = kv_cache.Sampler(0.9, 5, 0.95, seed=4)
    plain, plain_cache = _generate(kind, model, prompts, n, monkeypatch, sampler=smp, eos_id=eos)
    if kind == "paged":
        plain_cache.sync()
    feeds = []
    real = ops.spec_feed_rows
    monkeypatch.setattr(ops, "spec_feed_rows", lambda *a, **kw: feeds.append(1) or real(*a, **kw))
    misses = [lambda r, b: (r + b) % (k + 1), lambda r, b: 0, lambda r, b: None, "lookup"]
    for miss in misses:
        stats = {}
        for graph in (False, True):
            drafter = None if miss == "lookup" else S.OracleDrafter(plain, S.VOCAB, miss)
            spec = kv_cache.Speculation(k=k, drafter=drafter, graph=graph)
            del feeds[:]
            got, cache = _generate(kind, model, prompts, n, monkeypatch, sampler=smp, eos_id=eos, speculate=spec)
            for g, w, p in zip(got, plain, prompts):
                assert g.dtype == w.dtype and g.device == p.device and torch.equal(g, w)
            stats[graph] = dict(spec.stats)
            assert len(feeds) == (spec.stats["rounds"] if graph else 0)            # every round took the fixed shape
            if kind == "paged":
                assert cache.pages_in_use() == plain_cache.pages_in_use()
                assert cache.host_lengths == plain_cache.host_lengths
                assert cache.lengths[:3].tolist() == [cache.host_lengths[q] for q in range(3)]
        assert stats[True] == stats[False] and stats[True]["rounds"] >= 1


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_a_round_that_does_not_fit_the_window_runs_eagerly(kind, monkeypatch):
    S.stub_steps(monkeypatch)
    model, k, n = S.Model(), 7, 14
    assert model.block_size == 64
    prompts = S.prompts(50, 20)
    smp = kv_cache.Sampler(0.9, 5, 0.95, seed=4)
    plain, _ = _generate(kind, model, prompts, n, monkeypatch, sampler=smp)
    calls = {"fixed": 0, "eager": 0}
    real_feed = ops.spec_feed_rows
    name = "append_ragged" if kind == "ragged" else "append_paged"
    real_append = getattr(kv_cache, name)

    def feed(*a, **kw):
        calls["fixed"] += 1
        return real_feed(*a, **kw)

    def append(*a, **kw):
        calls["eager"] += 1
        return real_append(*a, **kw)

    monkeypatch.setattr(ops, "spec_feed_rows", feed)
    monkeypatch.setattr(kv_cache, name, append)
    for miss in (lambda r, b: None, lambda r, b: (r + b) % (k + 1)):
        calls.update(fixed=0, eager=0)
        spec = kv_cache.Speculation(k=k, drafter=S.OracleDrafter(plain, S.VOCAB, miss), graph=True)
        got, _ = _generate(kind, model, prompts, n, monkeypatch, sampler=smp, speculate=spec)
        assert all(torch.equal(g, w) for g, w in zip(got, plain))
        # 50 + 8 fits the window; from length 57 on the long prompt's rounds cannot
        assert calls["fixed"] >= 1 and calls["eager"] >= 1, calls
        assert calls["fixed"] + calls["eager"] == spec.stats["rounds"]


def test_flag_off_runs_nothing_of_it(monkeypatch):
    S.stub_steps(monkeypatch)
    seen = []
    for name in ("spec_feed_rows", "spec_commit_lengths"):
        monkeypatch.setattr(ops, name, lambda *a, **kw: seen.append(1))
    monkeypatch.setattr(kv_cache, "SpecRound", lambda *a, **kw: seen.append(1))
    model, prompts, smp = S.Model(), S.prompts(6, 3, 8), kv_cache.Sampler(0.9, 5, 0.95, seed=4)
    for kind in ("ragged", "paged"):
        plain, _ = _generate(kind, model, prompts, 9, monkeypatch, sampler=smp)
        got, _ = _generate(kind, model, prompts, 9, monkeypatch, sampler=smp, speculate=kv_cache.Speculation(k=3))
        assert all(torch.equal(g, w) for g, w in zip(got, plain))
    assert not seen
