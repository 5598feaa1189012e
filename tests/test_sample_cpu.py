"""CPU checks of the row sampler: Philox4x32-10 known answers (the tests' numpy one and
``ops.philox4x32_10``), ``dta_sample_rows`` in the header and the built library inside ABI 9 with the
struct laid out as ``_lib.SampleRowsArgs`` says, every validation code it returns before a launch,
``ops.sample_rows_reference`` against a plain sort-based top-k / top-p filter and on ties, and the
``sampler`` argument of the generate loops on CPU tensors (the model step stubbed)."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _sample_oracle as orc
from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for counter, key, out in KNOWN:
        assert orc.philox4x32_10(counter, key) == out
    counter = torch.tensor([c for c, _, _ in KNOWN], dtype=torch.int64)
    key = torch.tensor([k for _, k, _ in KNOWN], dtype=torch.int64)
    assert ops.philox4x32_10(counter, key).tolist() == [list(o) for _, _, o in KNOWN]
    # the uniform: counter (offset lo, offset hi, stream lo, stream hi), key (seed lo, seed hi)
    seed, strm, off = 0x299f31d0a4093822, 0x0370734413198a2e, -0x7a5cf72cdbc09578        # off: 0x85a308d3243f6a88 as int64
    u = ops.sample_uniform(seed, torch.tensor([strm]), torch.tensor([off]))
    assert u.item() == (0xd16cfe09 >> 8) * 2.0 ** -24 == orc.uniform(seed, strm, off)
    assert 0.0 <= u.item() < 1.0


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_sample_args_match_the_header():
    cname, py = "dta_sample_rows_args", _lib.SampleRowsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += [f'  printf("symbols declared %zu\\n", sizeof(dta_sample_rows((const {cname}*)0, (void*)0)) / sizeof(int));',
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
    """A call that passes every host check at R = 0: no pointer is read, nothing is launched."""
    a = _lib.SampleRowsArgs()
    a.dtype, a.R, a.V, a.row_stride = _lib.DTA_BF16, 0, 100, 100
    a.temperature, a.top_k, a.top_p, a.seed = 1.0, 0, 1.0, 7
    buf = (ctypes.c_int64 * 8)()
    a.logits = a.token_out = ctypes.addressof(buf)
    a._keep = buf
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_built_library_exports_the_sampler_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.SAMPLE_EXPORTS == ("dta_sample_rows",)
    assert "dta_sample_rows" in _lib.EXPORTS and hasattr(lib, "dta_sample_rows")
    assert ops.sample_supported() is True

    class _Old:
        dta_kv_step_rows = None
    assert not _lib.sample_symbols(_Old())

    fn = lib.dta_sample_rows
    here = _args().logits
    assert fn(None, None) == -1
    assert fn(ctypes.byref(_args()), None) == 0                                       # R = 0: valid, no launch
    assert fn(ctypes.byref(_args(logits=None, token_out=None)), None) == 0            # ... and no pointer needed
    assert fn(ctypes.byref(_args(V=1 << 20)), None) == 0
    assert fn(ctypes.byref(_args(V=(1 << 20) + 1)), None) == -2
    per_row = dict(temperature_dev=here, top_k_dev=here, top_p_dev=here, stream_dev=here, offset_dev=here,
                   logprob_out=here)
    assert fn(ctypes.byref(_args(**per_row)), None) == 0
    nan = float("nan")
    for bad in (dict(R=-1), dict(V=0), dict(V=-5), dict(dtype=3), dict(dtype=-1), dict(temperature=nan), dict(top_p=nan),
                dict(R=1, logits=None), dict(R=1, token_out=None),
                dict(temperature_dev=here + 2), dict(top_k_dev=here + 1), dict(top_p_dev=here + 2),
                dict(logprob_out=here + 2), dict(stream_dev=here + 4), dict(offset_dev=here + 4)):
        assert fn(ctypes.byref(_args(**bad)), None) == -1, bad
    assert fn(ctypes.byref(_args(temperature=float("inf"), top_p=-1.0, top_k=-3)), None) == 0   # odd, not invalid


def _sorted_filter(x, T, k, p):
    """The usual filter: top-k by the k-th value, then ascending cumulative probability <= 1 - p removed."""
    z = x.double() / T
    if 0 < k < x.numel():
        z = z.masked_fill(z < z.topk(k).values[-1], float("-inf"))
    if 0 < p < 1:
        zs, order = torch.sort(z)
        drop = F.softmax(zs, dim=-1).cumsum(-1) <= 1 - p
        drop[-1] = False
        z = z.masked_fill(torch.zeros_like(drop).scatter(0, order, drop), float("-inf"))
    return z > float("-inf")


def _tie_free(seed, V):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * 4
    assert x.unique().numel() == V
    return x


@pytest.mark.parametrize("V", [7, 257, 4099])
def test_reference_keeps_what_the_sorted_filter_keeps(V):
    for seed, (T, k, classes) in enumerate([(1.0, 0, 1), (1.0, 0, 3), (0.7, 0, 4), (1.5, 5, 2), (0.7, 50, 5), (1.0, V, 3)]):
        x = _tie_free(100 * V + seed, V)
        p = orc.midpoint_p(x.numpy(), T, k, classes)
        row = orc.Row(x.numpy(), T, k, p)
        assert row.margin >= 16 * row.E and row.margin > 1e-4 * row.Z, (V, seed, row.margin)   # every row: none dropped
        want = _sorted_filter(x, T, k, p)
        got = ops.sample_rows_reference(x[None], T, k, p, kept_only=True)[0]
        assert torch.equal(got, want) and int(got.sum()) == classes
        assert np.array_equal(row.kept, want.numpy())
        # top-k alone and top-p off
        got = ops.sample_rows_reference(x[None], T, k, 1.0, kept_only=True)[0]
        assert torch.equal(got, _sorted_filter(x, T, k, 1.0)) and int(got.sum()) == (k if 0 < k < V else V)
    # per-row parameters in one call
    xs = torch.stack([_tie_free(9 * V + i, V) for i in range(3)])
    Ts, ks = [1.0, 0.7, 1.5], [0, 3, 0]
    ps = [orc.midpoint_p(xs[i].numpy(), Ts[i], ks[i], 2) for i in range(3)]
    got = ops.sample_rows_reference(xs, torch.tensor(Ts), torch.tensor(ks), torch.tensor(ps), kept_only=True)
    for i in range(3):
        assert torch.equal(got[i], _sorted_filter(xs[i], Ts[i], ks[i], ps[i]))


def test_reference_on_ties_and_edges():
    ref = ops.sample_rows_reference
    # bf16-rounded logits: a tie class straddling k is kept whole
    x = torch.tensor([1.0, 3.0, 2.0, 3.0, 2.0, 2.0, 0.5, -1.0]).bfloat16()
    for k, n in ((1, 2), (2, 2), (3, 5), (4, 5), (5, 5), (6, 6), (7, 7)):
        kept = ref(x[None], 1.0, k, 1.0, kept_only=True)[0]
        assert int(kept.sum()) == n and np.array_equal(kept.numpy(), orc.Row(x.float().numpy(), 1.0, k, 1.0).kept), k
    # top-p: ties are in or out together; the maximum class is always kept
    w = torch.exp(x.double() - 3.0)
    p_two, p_five = float(w[[1, 3]].sum() / w.sum()) * 0.5, float((w[[1, 3]].sum() + 1.5 * w[2]) / w.sum())
    assert int(ref(x[None], 1.0, 0, p_two, kept_only=True).sum()) == 2
    assert int(ref(x[None], 1.0, 0, p_five, kept_only=True).sum()) == 5
    assert int(ref(x[None], 1.0, 0, 1e-30, kept_only=True).sum()) == 2
    # all-equal rows: everything is kept, by any filter, and the draw is the CDF's
    eq = torch.full((4, 9), -2.5)
    assert bool(ref(eq, 0.7, 3, 0.5, kept_only=True).all())
    off = torch.arange(4)
    tok, lp = ref(eq, 0.7, 3, 0.5, seed=11, offset=off, return_logprobs=True)
    for r in range(4):
        orc.check_row(eq[r].numpy(), 0.7, 3, 0.5, 11, r, r, tok[r], lp[r].item())
        assert abs(lp[r].item() + np.log(9)) < 1e-6
    # V = 1, one-hot with -inf elsewhere, greedy ties, degenerate rows
    assert ref(torch.tensor([[0.3]]), 1.0, 5, 0.2).tolist() == [0]
    hot = torch.full((3, 11), float("-inf"))
    hot[0, 4], hot[1, 0], hot[2, 10] = 1.0, -7.0, 3e38
    tok, lp = ref(hot, 1.3, 0, 1.0, seed=3, return_logprobs=True)
    assert tok.tolist() == [4, 0, 10] and lp.tolist() == [0.0, 0.0, 0.0]
    assert ref(torch.tensor([[1.0, 5.0, 5.0, -0.0, 5.0]]), 0.0).tolist() == [1]
    assert ref(torch.tensor([[-0.0, 0.0, -1.0]]), -1.0).tolist() == [0]                 # -0 == +0: the lowest index
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[0.0, nan, 1.0], [0.0, inf, 1.0], [-inf, -inf, -inf], [0.0, 1.0, 2.0]])
    for T in (0.0, 1.0):
        tok, lp = ref(bad, T, return_logprobs=True)
        assert tok[:3].tolist() == [-1, -1, -1] and 0 <= tok[3] < 3
        assert torch.isnan(lp[:3]).all() and torch.isfinite(lp[3])
    # NaN per-row parameters: greedy, and top-p off
    tok = ref(torch.tensor([[0.0, 2.0, 1.0]] * 2), torch.tensor([nan, 1.0]), 0, torch.tensor([0.5, nan]), seed=1)
    assert tok[0] == 1
    # shapes: (..., V) in, (...) out; ops.sample_rows falls back to the reference on CPU tensors
    x3 = torch.randn(2, 3, 33)
    tok, lp = ops.sample_rows(x3, 0.9, 4, 0.8, seed=2, return_logprobs=True)
    assert tok.shape == lp.shape == (2, 3) and tok.dtype == torch.int64 and lp.dtype == torch.float32
    assert torch.equal(tok, ref(x3, 0.9, 4, 0.8, seed=2))
    assert torch.equal(tok.reshape(-1)[4:5], ref(x3.reshape(6, 33)[4:5], 0.9, 4, 0.8, seed=2, stream=torch.tensor([4])))
    with pytest.raises(RuntimeError):
        ops.sample_rows(x3, float("nan"))
    with pytest.raises(RuntimeError):
        ops.sample_rows(x3.long())


# ---------------------------------------------------------------- plumbing ---
VOCAB = 13


class _Model:
    block_size = 64


@pytest.fixture
def stubbed(monkeypatch):
    """The ragged model step replaced by a table lookup, so the loops run on CPU tensors: a sequence's
    logits are a function of its last real token and its position."""
    table = torch.randn(VOCAB, VOCAB, generator=torch.Generator().manual_seed(5)) * 3

    def ragged(model, idx, cache, pos, counts, gather=None, one_row=False):
        if gather is not None:                                  # the prefill: each sequence's last real row
            last = idx.gather(1, gather[:, None])[:, 0]
            return table[last] + 0.01 * gather[:, None]
        return (table[idx[:, 0]] + 0.01 * pos[:, None])[:, None, :]

    monkeypatch.setattr(kv_cache, "_ragged_model_step", ragged)
    return table


def _prompts(*lens):
    return [(torch.arange(n, dtype=torch.long) * 7 + n) % VOCAB for n in lens]


def test_sampler_object():
    s = kv_cache.Sampler(0.8, 50, 0.9, seed=1)
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (0.8, 50, 0.9, 1)
    d = kv_cache.Sampler()
    assert (d.temperature, d.top_k, d.top_p, d.seed) == (1.0, 0, 1.0, 0)
    with pytest.raises(AttributeError):
        s.seed = 2
    with pytest.raises(ValueError):
        kv_cache.Sampler(temperature=float("nan"))


def test_greedy_sampler_is_the_argmax_loop(stubbed):
    model, prompts, n = _Model(), _prompts(3, 9, 5), 6
    got = kv_cache.generate_ragged(model, prompts, n, sampler=kv_cache.Sampler(temperature=0))
    cache = kv_cache.RaggedKVCache()
    logits = kv_cache.prefill_ragged(model, prompts, cache)
    toks = []
    for step in range(n):
        toks.append(logits.argmax(dim=-1, keepdim=True))
        if step + 1 < n:
            logits = kv_cache.decode_ragged(model, toks[-1], cache)
    toks = torch.cat(toks, dim=1)
    for b, p in enumerate(prompts):
        assert torch.equal(got[b], torch.cat([p, toks[b]]))


def test_without_a_sampler_the_tokens_are_the_reference_loop(stubbed):
    model, prompts, n = _Model(), _prompts(4, 2, 7), 8
    torch.manual_seed(21)
    got = kv_cache.generate_ragged(model, prompts, n, sampler=None)
    torch.manual_seed(21)
    also = kv_cache.generate_ragged(model, prompts, n)
    torch.manual_seed(21)
    cache = kv_cache.RaggedKVCache()
    logits = kv_cache.prefill_ragged(model, prompts, cache)
    toks = []
    for step in range(n):
        toks.append(torch.multinomial(F.softmax(logits, dim=-1), num_samples=1))
        if step + 1 < n:
            logits = kv_cache.decode_ragged(model, toks[-1], cache)
    toks = torch.cat(toks, dim=1)
    for b, p in enumerate(prompts):
        assert torch.equal(got[b], torch.cat([p, toks[b]])) and torch.equal(also[b], got[b])


def test_a_sequence_gets_the_same_streams_and_offsets_alone_and_in_a_batch(stubbed, monkeypatch):
    model, n = _Model(), 5
    a, x, y = _prompts(6, 3, 8)
    calls = []
    real = ops.sample_rows

    def spy(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs=False):
        strm = torch.arange(logits.shape[0]) if stream is None else stream
        calls.append((strm.tolist(), offset.tolist(), seed))
        return real(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs)

    monkeypatch.setattr(ops, "sample_rows", spy)
    s = kv_cache.Sampler(0.9, 5, 0.95, seed=4)
    alone = kv_cache.generate_ragged(model, [a], n, sampler=s, streams=[7])[0]
    pairs_alone = [(c[0][0], c[1][0]) for c in calls]
    calls.clear()
    batch = kv_cache.generate_ragged(model, [x, a, y], n, sampler=s, streams=[3, 7, 5])
    pairs_batch = [(c[0][1], c[1][1]) for c in calls]
    assert pairs_alone == pairs_batch == [(7, t) for t in range(n)]
    assert all(c[2] == 4 for c in calls)
    assert torch.equal(alone, batch[1])                       # and so the same tokens
    # the default stream is the index in the call
    calls.clear()
    kv_cache.generate_ragged(model, [x, a, y], 2, sampler=s)
    assert [c[0] for c in calls] == [[0, 1, 2]] * 2 and [c[1] for c in calls] == [[0] * 3, [1] * 3]
    # a second seed gives other tokens, the same seed the same
    again = kv_cache.generate_ragged(model, [a], n, sampler=s, streams=[7])[0]
    other = kv_cache.generate_ragged(model, [a], 24, sampler=kv_cache.Sampler(0.9, 5, 0.95, seed=5), streams=[7])[0]
    same = kv_cache.generate_ragged(model, [a], 24, sampler=s, streams=[7])[0]
    assert torch.equal(again, alone) and not torch.equal(other, same)
    with pytest.raises(ValueError):
        kv_cache.generate_ragged(model, [a], 2, sampler=s, streams=[1, 2])
