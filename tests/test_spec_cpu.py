"""CPU checks of speculative decoding: ``dta_spec_accept_draft`` in the header and the built library inside
ABI 9 with the struct laid out as ``_lib.SpecAcceptDraftArgs`` says, every validation code it returns before
a launch, ``ops.spec_accept_draft_reference`` against a brute-force reading of the definition (random
small-alphabet histories and hand cases), and the ``speculate`` argument of ``generate_ragged`` /
``generate_paged`` on CPU tensors with the model step stubbed: the tokens are the plain sampler loop's."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

import _spec as S
from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_spec_args_match_the_header():
    cname, py = "dta_spec_accept_draft_args", _lib.SpecAcceptDraftArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += [f'  printf("symbols declared %zu\\n", sizeof(dta_spec_accept_draft((const {cname}*)0, (void*)0)) / sizeof(int));',
              '  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
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
    assert got[("symbols", "declared")] == 1
    assert got[(cname, "sizeof")] == ctypes.sizeof(py)
    bad = [(f[0], got[(cname, f[0])], getattr(py, f[0]).offset) for f in py._fields_
           if got[(cname, f[0])] != getattr(py, f[0]).offset]
    assert not bad, bad


def _args(**kw):
    """A call that passes every host check at B = 0: no pointer is read, nothing is launched."""
    a = _lib.SpecAcceptDraftArgs()
    a.B, a.Tn, a.K, a.cap, a.t_cap, a.ngram_min, a.ngram_max, a.eos_id = 0, 4, 3, 64, 64, 1, 3, -1
    a.hist_stride, a.draft_stride, a.tok_stride = 64, 3, 4
    buf = (ctypes.c_int64 * 8)()
    here = ctypes.addressof(buf)
    a.hist = a.hlen_dev = a.remaining_dev = a.draft = a.dcnt_dev = a.tok = a.result_out = here
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_kernel_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.SPEC_EXPORTS == ("dta_spec_accept_draft",)
    assert "dta_spec_accept_draft" in _lib.EXPORTS and hasattr(lib, "dta_spec_accept_draft")
    assert ops.spec_supported() is True

    class _Old:
        dta_sample_rows = None
    assert not _lib.spec_symbols(_Old())

    fn = lib.dta_spec_accept_draft
    here = _args().hist
    assert fn(None, None) == -1
    assert fn(ctypes.byref(_args()), None) == 0                                    # B = 0: valid, no launch
    for ok in (dict(K=1, Tn=2, draft_stride=1), dict(K=7, Tn=8, tok_stride=8, draft_stride=7), dict(Tn=0, tok=None),
               dict(ngram_min=0), dict(ngram_min=8, ngram_max=8), dict(eos_id=5), dict(hist_stride=100)):
        assert fn(ctypes.byref(_args(**ok)), None) == 0, ok
    for bad in (dict(K=0), dict(K=8, draft_stride=8), dict(B=-1), dict(Tn=-1), dict(Tn=5, tok_stride=5),
                dict(ngram_min=3, ngram_max=2), dict(ngram_max=9), dict(ngram_min=-1), dict(ngram_min=0, ngram_max=0),
                dict(cap=0), dict(t_cap=0), dict(cap=(1 << 30) + 1, hist_stride=1 << 31),
                dict(hist_stride=63), dict(draft_stride=2), dict(tok_stride=3),
                dict(hist=None), dict(hlen_dev=None), dict(remaining_dev=None), dict(draft=None), dict(dcnt_dev=None),
                dict(tok=None), dict(result_out=None),
                dict(hist=here + 2), dict(hlen_dev=here + 1), dict(remaining_dev=here + 2), dict(draft=here + 2),
                dict(dcnt_dev=here + 3), dict(tok=here + 4), dict(result_out=here + 2)):
        assert fn(ctypes.byref(_args(**bad)), None) == -1, bad


# ------------------------------------------------------------------ the reference ---
@pytest.mark.parametrize("nmin,nmax", [(1, 1), (1, 3), (2, 8)])
def test_reference_is_the_definition_on_random_histories(nmin, nmax):
    seen = set()
    for K in range(1, 8):
        for seed, t_cap in enumerate((40, 1 << 20)):
            st = S.random_state(24, [1, 2, 3, 5, 9, 17, 30, 38], 40, 3, K, 1000 * K + seed, eos_rate=0.05)
            seen |= {(K, m) for m in S.check_against_brute_force(st, 2 if seed else -1, K, nmin, nmax, t_cap)}
    # finished rows, rejections and acceptances all occurred (test_reference_hand_cases walks every a = 0 .. K)
    assert {m for k, m in seen if k == 7} >= {0, 1, 2, 3}


def _one(hist, remaining, draft, dcnt, tok, K=3, nmin=1, nmax=3, t_cap=1 << 20, eos_id=-1, cap=None):
    """One row through the reference and the brute force; returns (m, dcnt, draft[:dcnt], hist[:hlen], remaining)."""
    cap = cap or len(hist) + 8
    h = hist + [99] * (cap - len(hist))
    d = draft + [77] * (K - len(draft))
    st = S.State(S.i32([h]), S.i32([len(hist)]), S.i32([remaining]), S.i32([d]), S.i32([dcnt]),
                 torch.tensor([tok], dtype=torch.int64) if tok else None)
    S.check_against_brute_force(st, eos_id, K, nmin, nmax, t_cap)
    res = st.run(ops.spec_accept_draft_reference, eos_id, K, nmin, nmax, t_cap)
    m, dc = res[0].tolist()
    L = int(st.hlen[0])
    assert st.hist[0, L:].tolist() == [99] * (cap - L) and st.draft[0, dc:].tolist() == d[dc:]
    return m, dc, st.draft[0, :dc].tolist(), st.hist[0, :L].tolist(), int(st.remaining[0])


def test_reference_hand_cases():
    # no match: the last token has no earlier occurrence
    assert _one([1, 2, 3, 4], 9, [], 0, [5])[:2] == (1, 0)
    # a match whose continuation runs into the end: 7 8 | 7 -> [8, 7], L - 1 - e = 2 < K
    assert _one([7, 8], 9, [], 0, [7])[:3] == (1, 2, [8, 7])
    # two matches of equal n: the latest wins
    assert _one([1, 5, 2, 1, 6, 2], 9, [], 0, [1], nmax=1)[:3] == (1, 3, [6, 2, 1])
    # a longer but earlier match wins over a later shorter one: ... 3 1 [4 4 4] ... 9 1 [5 5] ... 3 | 1
    assert _one([3, 1, 4, 4, 4, 9, 1, 5, 5, 3], 9, [], 0, [1], nmax=3)[:3] == (1, 3, [4, 4, 4])
    assert _one([3, 1, 4, 4, 4, 9, 1, 5, 5, 3], 9, [], 0, [1], nmax=1)[:3] == (1, 3, [5, 5, 3])
    # ngram_min = 2 refuses a one-token match
    assert _one([1, 5, 2, 6], 9, [], 0, [1], nmin=2, nmax=3)[:2] == (1, 0)
    # clipped by remaining - 1 and by t_cap - L
    assert _one([1, 2, 3, 4, 5], 3, [], 0, [1])[:3] == (1, 1, [2])
    assert _one([1, 2, 3, 4, 5], 2, [], 0, [1])[:2] == (1, 0)
    assert _one([1, 2, 3, 4, 5], 9, [], 0, [1], t_cap=8)[:3] == (1, 2, [2, 3])
    assert _one([1, 2, 3, 4, 5], 9, [], 0, [1], t_cap=6)[:2] == (1, 0)
    # every acceptance count a = 0 .. K, and m cut by remaining
    for K in (1, 3, 7):
        d = list(range(10, 10 + K))
        for a in range(K + 1):
            tok = d[:a] + [50] * (K + 1 - a)
            m, _, _, h, rem = _one([0, 1], 20, d, K, tok, K=K)
            assert (m, h, rem) == (a + 1, [0, 1] + tok[:a + 1], 20 - a - 1)
            assert _one([0, 1], 2, d, K, tok, K=K)[0] == min(a + 1, 2)
    # a short draft: only its dcnt leading entries count
    assert _one([0, 1], 20, [10, 11, 12], 1, [10, 11, 12, 13])[0] == 2
    # EOS inside the accepted prefix ends the sequence there; so does the sampler's -1
    m, dc, _, h, rem = _one([0, 1], 20, [10, 4, 12], 3, [10, 4, 12, 13], eos_id=4)
    assert (m, dc, h, rem) == (2, 0, [0, 1, 10, 4], 0)
    m, dc, _, h, rem = _one([0, 1], 20, [10, 11, 12], 3, [10, -1, 12, 13])
    assert (m, dc, h, rem) == (2, 0, [0, 1, 10, -1], 0)
    # no rows to accept: only a draft
    assert _one([7, 8, 7], 9, [], 0, None)[:4] == (0, 2, [8, 7], [7, 8, 7])


def test_finished_rows_are_untouched():
    st = S.random_state(6, [5, 9], 40, 3, 4, seed=3)
    st.remaining[:] = S.i32([0, 4, 0, -3, 2, 0])
    st.hist.view(torch.uint8)[0] = 0xFF                     # poison: not one byte of a finished row changes
    before = st.clone()
    res = st.run(ops.spec_accept_draft_reference, -1, 4, 1, 3, 64)
    for b in (0, 2, 3, 5):
        assert res[b].tolist() == [0, 0]
        for new, old in zip(st.tensors()[:5], before.tensors()[:5]):
            assert torch.equal(new[b:b + 1].contiguous().view(torch.uint8), old[b:b + 1].contiguous().view(torch.uint8))
    assert res[1, 0] >= 1 and res[4, 0] >= 1


def test_wrappers_reject_bad_arguments():
    st = S.random_state(2, [5], 16, 3, 3, seed=1)
    for kw in (dict(K=0), dict(K=8), dict(nmin=3, nmax=2), dict(nmax=9)):
        a = dict(K=3, nmin=1, nmax=3)
        a.update(kw)
        with pytest.raises(ValueError):
            st.clone().run(ops.spec_accept_draft, -1, a["K"], a["nmin"], a["nmax"], 64)
    with pytest.raises(ValueError):
        ops.spec_accept_draft(st.hist.long(), st.hlen, st.remaining, st.draft, st.dcnt, st.tok, -1, 3, 1, 3, 64)
    with pytest.raises(ValueError):
        ops.spec_accept_draft(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, st.tok.int(), -1, 3, 1, 3, 64)


# ------------------------------------------------------------------ the loops ---
def test_speculation_object():
    s = kv_cache.Speculation()
    assert (s.k, s.ngram_max, s.ngram_min, s.drafter) == (4, 3, 1, None)
    assert s.stats == dict(rounds=0, drafted=0, accepted=0, emitted=0)
    with pytest.raises(AttributeError):
        s.k = 2
    for bad in (dict(k=0), dict(k=8), dict(ngram_min=0), dict(ngram_min=4, ngram_max=3), dict(ngram_max=9),
                dict(drafter=object())):
        with pytest.raises(ValueError):
            kv_cache.Speculation(**bad)


def test_speculate_value_errors(monkeypatch):
    S.stub_steps(monkeypatch)
    model, prompts, spec, sampler = S.Model(), S.prompts(3, 5), kv_cache.Speculation(), kv_cache.Sampler(0)
    for gen in (kv_cache.generate_ragged, kv_cache.generate_paged):
        with pytest.raises(ValueError, match="sampler"):
            gen(model, prompts, 4, speculate=spec)
        with pytest.raises(ValueError):
            gen(model, prompts, 4, sampler=sampler, speculate="yes")
        with pytest.raises(ValueError, match="block_size"):
            gen(model, S.prompts(60), 5, sampler=sampler, speculate=spec)
    with pytest.raises(ValueError, match="n_samples"):
        kv_cache.generate_paged(model, prompts, 4, sampler=sampler, speculate=spec, n_samples=2)
    with pytest.raises(ValueError, match="shared_decode"):
        kv_cache.generate_paged(model, prompts, 4, sampler=sampler, speculate=spec, shared_decode=True)


def _generate(kind, model, prompts, n, monkeypatch, **kw):
    """(outputs, pages in use after the call or None)."""
    if kind == "ragged":
        return kv_cache.generate_ragged(model, prompts, n, **kw), None
    monkeypatch.setattr(kv_cache, "PagedKVCache", S.RecordingPagedCache)
    out = kv_cache.generate_paged(model, prompts, n, page_size=32, **kw)
    return out, S.RecordingPagedCache.last


SAMPLERS = {"greedy": dict(temperature=0.0), "filtered": dict(temperature=0.9, top_k=5, top_p=0.95, seed=4)}
# name: (prompt lengths, new tokens, eos_id, k); block_size is 64
CASES = {"plain": ((3, 9, 5), 12, None, 3),
         "eos_mid_round": ((3, 9, 5), 20, 4, 3),
         "not_a_multiple_of_k_plus_1": ((6, 2, 11, 4), 14, None, 4),
         "k7": ((6, 2, 11, 4), 23, None, 7),
         "one_short_of_block_size": ((63, 40, 5), 1, None, 3),
         "up_to_block_size": ((50, 41, 57), 7, None, 3)}


@pytest.mark.parametrize("kind", ["ragged", "paged"])
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_speculative_tokens_are_the_plain_loops(case, sampler, kind, monkeypatch):
    S.stub_steps(monkeypatch)
    lens, n, eos, k = CASES[case]
    model, prompts, smp = S.Model(), S.prompts(*lens), kv_cache.Sampler(**SAMPLERS[sampler])
    plain, plain_cache = _generate(kind, model, prompts, n, monkeypatch, sampler=smp, eos_id=eos)
    if eos is not None:
        cut = [len(o) - len(p) for o, p in zip(plain, prompts)]
        assert any(1 < c < n for c in cut), cut            # the case does cut a sequence short
    # an oracle drafter with the miss walking through every index 0 .. k (k: all accepted), and the lookup
    drafters = [S.OracleDrafter(plain, S.VOCAB, lambda r, b: (r + b) % (k + 1)),
                S.OracleDrafter(plain, S.VOCAB, lambda r, b: None), None]
    for drafter in drafters:
        spec = kv_cache.Speculation(k=k, drafter=drafter)
        got, cache = _generate(kind, model, prompts, n, monkeypatch, sampler=smp, eos_id=eos, speculate=spec)
        assert len(got) == len(plain)
        for g, w, p in zip(got, plain, prompts):
            assert g.dtype == w.dtype and g.device == p.device and torch.equal(g, w)
        st = spec.stats
        assert st["emitted"] == sum(len(o) - len(p) for o, p in zip(plain, prompts))
        assert 0 <= st["accepted"] <= st["drafted"]
        if kind == "paged":
            # a plain run that an eos cut short holds pages for its upper bound until it syncs
            plain_cache.sync()
            assert cache.pages_in_use() == plain_cache.pages_in_use()
            assert cache.host_lengths == plain_cache.host_lengths
    if n > 1 and eos is None:                               # all drafts right: every round emits its k + 1
        assert drafters[1].round >= 1 and spec.stats["rounds"] <= n
        full = kv_cache.Speculation(k=k, drafter=S.OracleDrafter(plain, S.VOCAB, lambda r, b: None))
        _generate(kind, model, prompts, n, monkeypatch, sampler=smp, speculate=full)
        assert full.stats["rounds"] == -(-(n - 1) // (k + 1)) and full.stats["accepted"] == full.stats["drafted"]


def test_stats_add_up(monkeypatch):
    S.stub_steps(monkeypatch)
    model, prompts, smp, n, k = S.Model(), S.prompts(4, 7), kv_cache.Sampler(0.9, 5, 0.95, seed=2), 17, 3
    plain = kv_cache.generate_ragged(model, prompts, n, sampler=smp)
    ms = []
    real = ops.spec_accept_draft

    def spy(*a, **kw):
        res = real(*a, **kw)
        ms.append(res[:, 0].tolist())
        return res

    monkeypatch.setattr(ops, "spec_accept_draft", spy)
    spec = kv_cache.Speculation(k=k, drafter=S.OracleDrafter(plain, S.VOCAB, lambda r, b: (2 * r + b) % (k + 2)))
    kv_cache.generate_ragged(model, prompts, n, sampler=smp, speculate=spec)
    st = spec.stats
    assert st["emitted"] == sum(map(sum, ms)) == 2 * n
    assert st["rounds"] == len(ms) - 1                      # the first call accepts the prefill's sample
    assert st["accepted"] == sum(m - 1 for row in ms[1:] for m in row if m) <= st["drafted"]
    assert {m for row in ms[1:] for m in row} >= {1, 2, 3, 4}
    # the stats are the last call's
    kv_cache.generate_ragged(model, prompts, 1, sampler=smp, speculate=spec)
    assert spec.stats == dict(rounds=0, drafted=0, accepted=0, emitted=2)


def test_emitted_tokens_are_drawn_from_the_plain_loops_streams_and_offsets(monkeypatch):
    S.stub_steps(monkeypatch)
    model, prompts, smp, n, k = S.Model(), S.prompts(6, 3, 8), kv_cache.Sampler(0.9, 5, 0.95, seed=4), 11, 3
    plain = kv_cache.generate_ragged(model, prompts, n, sampler=smp, streams=[3, 7, 5])
    calls, ms = [], []
    real, real_accept = ops.sample_rows, ops.spec_accept_draft

    def spy(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs=False):
        rows = logits.reshape(-1, logits.shape[-1]).shape[0]
        calls.append((stream.reshape(len(prompts), -1).tolist(), offset.reshape(len(prompts), -1).tolist(), seed))
        assert stream.numel() == offset.numel() == rows
        return real(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs)

    def spy_accept(*a, **kw):
        res = real_accept(*a, **kw)
        ms.append(res[:, 0].tolist())
        return res

    monkeypatch.setattr(ops, "sample_rows", spy)
    monkeypatch.setattr(ops, "spec_accept_draft", spy_accept)
    spec = kv_cache.Speculation(k=k, drafter=S.OracleDrafter(plain, S.VOCAB, lambda r, b: (r + 2 * b) % (k + 1)))
    got = kv_cache.generate_ragged(model, prompts, n, sampler=smp, streams=[3, 7, 5], speculate=spec)
    assert all(torch.equal(g, w) for g, w in zip(got, plain))
    assert len(calls) == len(ms) and all(c[2] == 4 for c in calls)
    for b, strm in enumerate([3, 7, 5]):
        pairs = [(s, o) for (streams, offsets, _), m in zip(calls, ms)
                 for s, o in list(zip(streams[b], offsets[b]))[:m[b]]]
        assert pairs == [(strm, t) for t in range(n)]
