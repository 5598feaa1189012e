"""CPU checks of the sampling penalties: ``dta_penalize_rows`` in the header and the built library inside ABI 9
with the struct laid out as ``_lib.PenalizeRowsArgs`` says, every validation code it returns before a launch,
``ops.penalize_rows_reference`` bit for bit against a pure-Python reading of the definition
(tests/_penalty.py), ``kv_cache.Penalties``, and the ``penalties`` argument of the generate loops on CPU
tensors with the model step stubbed: bans hold, a large frequency penalty makes tokens distinct, and
speculative rounds emit the plain loop's tokens."""
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _penalty as P
import _spec as S
from differential_transformer_replication_amd import _lib, kv_cache, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2


# ------------------------------------------------------------------ the ABI ---
@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_args_match_the_header():
    cname, py = "dta_penalize_rows_args", _lib.PenalizeRowsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {",
             f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += [f'  printf("symbols declared %zu\\n", sizeof(dta_penalize_rows((const {cname}*)0, (void*)0)) / sizeof(int));',
              '  printf("query declared %zu\\n", sizeof(dta_penalize_rows_workspace_bytes(1, 1)) / sizeof(size_t));',
              '  printf("lds max %d\\n", DTA_PENALTY_LDS_MAX_V);',
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
    assert got[("symbols", "declared")] == 1 and got[("query", "declared")] == 1
    assert got[("lds", "max")] == ops.PENALTY_LDS_MAX_V
    assert got[(cname, "sizeof")] == ctypes.sizeof(py)
    bad = [(f[0], got[(cname, f[0])], getattr(py, f[0]).offset) for f in py._fields_
           if got[(cname, f[0])] != getattr(py, f[0]).offset]
    assert not bad, bad


BASE = 0x100000                     # fake device addresses, 16-byte aligned, never dereferenced
BIG = ops.PENALTY_LDS_MAX_V + 1


def _args(**kw):
    """A call that passes every host check with B = 0: no pointer is read, nothing is launched."""
    a = _lib.PenalizeRowsArgs()
    a.dtype, a.B, a.Tn, a.V, a.cap, a.K = _lib.DTA_BF16, 0, 4, 1000, 64, 3
    a.row_stride, a.out_stride, a.hist_stride, a.draft_stride, a.bias_stride = 1000, 1000, 64, 3, 0
    (a.logits, a.out, a.hist, a.hlen_dev, a.gen_start_dev, a.draft, a.dcnt_dev, a.repetition_dev, a.frequency_dev,
     a.presence_dev, a.floor_gap_dev, a.bias, a.workspace) = (BASE + (i << 16) for i in range(13))
    a.repetition, a.frequency, a.presence, a.floor_gap = 1.2, 0.5, 0.25, -3.0
    a.workspace_bytes = 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


NAN = float("nan")
ACCEPTED = [dict(), dict(B=2, Tn=0), dict(K=0, draft=None, dcnt_dev=None, draft_stride=0), dict(K=7, draft_stride=7),
            dict(gen_start_dev=None), dict(bias=None), dict(bias_stride=1000), dict(row_stride=5000, out_stride=1001),
            dict(repetition=0.5), dict(floor_gap=1.0), dict(floor_gap=float("-inf")), dict(dtype=_lib.DTA_F32),
            dict(V=1 << 20, row_stride=1 << 20, out_stride=1 << 20), dict(logits=BASE + 2),
            dict(V=BIG, row_stride=BIG, out_stride=BIG, workspace=None),      # R == 0 needs no workspace
            dict(logits=None, out=None, hist=None, hlen_dev=None)]            # R == 0 reads no pointer
REJECTED = [  # one per line of the header's error list
    (dict(B=-1), INVALID), (dict(Tn=-1), INVALID), (dict(B=1 << 20, Tn=1 << 12), INVALID), (dict(V=0), INVALID),
    (dict(dtype=3), INVALID), (dict(dtype=-1), INVALID),
    (dict(cap=0, hist_stride=0), INVALID), (dict(cap=(1 << 30) + 1, hist_stride=1 << 31), INVALID),
    (dict(K=-1), INVALID), (dict(K=8, draft_stride=8), INVALID),
    (dict(row_stride=999), INVALID), (dict(out_stride=999), INVALID), (dict(hist_stride=63), INVALID),
    (dict(draft_stride=2), INVALID), (dict(bias_stride=999), INVALID),
    (dict(B=1, logits=None), INVALID), (dict(B=1, out=None), INVALID), (dict(B=1, hist=None), INVALID),
    (dict(B=1, hlen_dev=None), INVALID),
    (dict(draft=None), INVALID), (dict(dcnt_dev=None), INVALID),
    (dict(logits=BASE + 1), INVALID), (dict(dtype=_lib.DTA_F32, logits=BASE + 2), INVALID), (dict(out=BASE + 0x10002), INVALID),
    (dict(hist=BASE + 0x20002), INVALID), (dict(hlen_dev=BASE + 0x30001), INVALID), (dict(gen_start_dev=BASE + 0x40002), INVALID),
    (dict(draft=BASE + 0x50002), INVALID), (dict(dcnt_dev=BASE + 0x60003), INVALID), (dict(repetition_dev=BASE + 0x70002), INVALID),
    (dict(frequency_dev=BASE + 0x80002), INVALID), (dict(presence_dev=BASE + 0x90002), INVALID),
    (dict(floor_gap_dev=BASE + 0xa0002), INVALID), (dict(bias=BASE + 0xb0002), INVALID), (dict(workspace=BASE + 0xc0002), INVALID),
    (dict(repetition=NAN), INVALID), (dict(frequency=NAN), INVALID), (dict(presence=NAN), INVALID), (dict(floor_gap=NAN), INVALID),
    (dict(repetition=0.0), INVALID), (dict(repetition=-1.5), INVALID),
    (dict(B=1, V=BIG, row_stride=BIG, out_stride=BIG, workspace=None), INVALID),
    (dict(B=1, V=BIG, row_stride=BIG, out_stride=BIG, workspace_bytes=4 * 4 * BIG - 1), INVALID),
    (dict(V=(1 << 20) + 1, row_stride=1 << 21, out_stride=1 << 21), UNSUPPORTED),
    (dict(V=(1 << 20) + 1, row_stride=1 << 21, out_stride=1 << 21, repetition=NAN), INVALID),   # INVALID comes first
]


def test_built_library_exports_the_kernel_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    assert _lib.PENALTY_EXPORTS == ("dta_penalize_rows", "dta_penalize_rows_workspace_bytes")
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in _lib.PENALTY_EXPORTS)
    assert ops.penalize_rows_supported() is True

    class _Old:
        dta_sample_rows = None
    assert not _lib.penalty_symbols(_Old())

    query = lib.dta_penalize_rows_workspace_bytes
    assert [query(R, V) for R, V in ((1, 1), (64, 12000), (8, BIG - 1), (0, BIG), (-1, BIG))] == [0] * 5
    assert query(1, BIG) == 4 * BIG and query(8, 1 << 20) == 8 * 4 << 20
    fn = lib.dta_penalize_rows
    assert fn(None, None) == INVALID
    for ok in ACCEPTED:
        assert fn(ctypes.byref(_args(**ok)), None) == OK, ok
    for bad, code in REJECTED:
        assert fn(ctypes.byref(_args(**bad)), None) == code, bad


# ------------------------------------------------------------------ the reference ---
@pytest.mark.parametrize("Tn", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1, 7, 33])
def test_reference_is_the_definition(V, B, Tn):
    for dtype in (torch.float32, torch.bfloat16):
        case = P.Case(B, Tn, V, dtype, seed=100 * V + 10 * B + Tn, draft=Tn > 1)
        outs = {}
        for name, kw in case.features().items():
            got = ops.penalize_rows_reference(**case.args("cpu", **kw))
            assert got.dtype == torch.float32 and got.shape == case.logits.shape
            want = case.brute(**kw)
            assert P.same_bits(got, want), (name, P.first_diff(got, want))
            assert P.same_bits(ops.penalize_rows(**case.args("cpu", **kw)), want)      # CPU tensors run the reference
            outs[name] = got
        if V == 33 and B == 3:
            assert all(not P.same_bits(outs[n], outs["none"]) for n in outs if n != "none")
        assert P.same_bits(outs["none"], case.logits.float())


@pytest.mark.parametrize("Tn", [1, 4])
@pytest.mark.parametrize("V", [7, 33])
def test_reference_clamps_are_the_definitions(V, Tn):
    """Eight sequences, so that every clamp is met: ``hlen`` above ``cap`` and negative, ``gen_start`` above
    ``hlen`` and negative, ``dcnt`` above K and negative."""
    case = P.Case(8, Tn, V, torch.float32, seed=7 * V + Tn, draft=Tn > 1)
    hl, gs = case.hlen.tolist(), case.gen_start.tolist()
    assert max(hl) > case.cap and min(hl) < 0 and min(gs) < 0
    assert any(g > h >= 0 for g, h in zip(gs, hl)) and any(0 < g < h <= case.cap for g, h in zip(gs, hl))
    if Tn > 1:
        assert max(case.dcnt.tolist()) > case.K and min(case.dcnt.tolist()) < 0
    for name, kw in case.features().items():
        got, want = ops.penalize_rows_reference(**case.args("cpu", **kw)), case.brute(**kw)
        assert P.same_bits(got, want), (name, P.first_diff(got, want))
    # gen_start above hlen counts nothing of the history (sequence 5: hlen cap - 1, gen_start cap + 9); at 0 all of it
    freq = ops.penalize_rows_reference(**case.args("cpu", frequency=0.7)).view(8, Tn, V)
    assert P.same_bits(freq[5, 0], case.logits.view(8, Tn, V)[5, 0])
    assert not P.same_bits(freq[1, 0], case.logits.view(8, Tn, V)[1, 0])
    rep = ops.penalize_rows_reference(**case.args("cpu", repetition=1.3)).view(8, Tn, V)
    assert not P.same_bits(rep[5, 0], case.logits.view(8, Tn, V)[5, 0])      # repetition still sees the history


def test_reference_edge_rows():
    ninf, nan = float("-inf"), float("nan")
    hist = P.i32([[2, 2, 5, 2, 0, 0, 0, 0]])
    one = lambda x, **kw: ops.penalize_rows_reference(torch.tensor([x]), hist, P.i32([4]), P.i32([1]), **kw)[0].tolist()   # noqa: E731
    # repetition sees the prompt too; frequency / presence count from gen_start on: token 2 twice, token 5 once
    x = [1.0, 1.0, 3.0, -3.0, 0.0, -1.0]
    assert one(x, repetition=2.0) == [1.0, 1.0, 1.5, -3.0, 0.0, -2.0]
    assert one(x, frequency=0.5) == [1.0, 1.0, 2.0, -3.0, 0.0, -1.5]
    assert one(x, presence=0.25) == [1.0, 1.0, 2.75, -3.0, 0.0, -1.25]
    # -0 is not positive: multiplied (and stays -0)
    z = ops.penalize_rows_reference(torch.tensor([[0.0, 0.0, -0.0]]), hist, P.i32([4]), repetition=2.0)
    assert z.view(torch.int32).tolist() == [[0, 0, -2 ** 31]]
    # the floor: keeps what is within gap of the maximum after the bias; ties in
    assert one([0.0, -1.0, -2.0, -1.0, 4.0, 0.0], bias=torch.tensor([0.0, 0, 0, 0, ninf, 0]), floor_gap=-1.0) == \
        [0.0, -1.0, ninf, -1.0, ninf, 0.0]
    # a row of -inf, and a +inf maximum: left as the bias made them
    assert one([ninf] * 6, floor_gap=-1.0, frequency=1.0) == [ninf] * 6
    assert one([float("inf"), 0, 0, 0, 0, 0], floor_gap=-1.0) == [float("inf"), 0, 0, 0, 0, 0]
    # a NaN is written through with its bits, and does not take part in the maximum
    odd = torch.from_numpy(np.array([[0x7FC12345, 0, 0xBF800000, 0xC0400000, 0, 0]], dtype=np.uint32).view(np.float32))
    got = ops.penalize_rows_reference(odd, hist, P.i32([4]), repetition=2.0, frequency=1.0,
                                      bias=torch.ones(6), floor_gap=-1.5)
    assert got.view(torch.int32)[0, 0] == 0x7FC12345 and got[0, 1:].tolist() == [1.0, ninf, ninf, 1.0, 0.0]
    # a NaN that the arithmetic makes (+inf on a banned column) stays a NaN through the floor, and is not the maximum
    made = ops.penalize_rows_reference(torch.tensor([[float("inf"), 1.0, 0.0, -5.0, 0.0, 0.0]]), hist, P.i32([0]),
                                       bias=torch.tensor([ninf, 0, 0, 0, 0, 0]), floor_gap=-2.0)[0]
    assert bool(torch.isnan(made[0])) and made[1:].tolist() == [1.0, 0.0, ninf, 0.0, 0.0]
    want = P.brute_force(np.array([[np.inf, 1, 0, -5, 0, 0]], dtype=np.float32), hist.tolist(), [0], None, None, None,
                         [1.0], [0.0], [0.0], [-2.0], np.array([[-np.inf, 0, 0, 0, 0, 0]], dtype=np.float32), 1)
    assert P.same_bits(made[None], torch.from_numpy(want))
    # floor_gap off: >= 0, -inf, None
    for gap in (0.0, 2.0, ninf, None):
        assert one(x, floor_gap=gap) == x
    # a draft prefix grows with the row index and stops at dcnt
    rows = ops.penalize_rows_reference(torch.zeros(4, 6), hist, P.i32([0]), None, P.i32([[1, 1, 3]]), P.i32([2]),
                                       frequency=1.0, rows_per_seq=4)
    assert rows.tolist() == [[0.0] * 6, [0, -1.0, 0, 0, 0, 0], [0, -2.0, 0, 0, 0, 0], [0, -2.0, 0, 0, 0, 0]]


def test_wrapper_rejects_bad_arguments():
    case = P.Case(2, 2, 7, torch.float32, seed=1)
    good = case.args("cpu")
    for bad in (dict(hist=case.hist.long()), dict(hlen=case.hlen[:1]), dict(gen_start=case.gen_start.float()),
                dict(draft=None), dict(dcnt=None), dict(draft=torch.zeros(2, 8, dtype=torch.int32)),
                dict(rows_per_seq=3), dict(rows_per_seq=0), dict(repetition=0.0), dict(repetition=float("nan")),
                dict(frequency=float("nan")), dict(presence=torch.zeros(3)), dict(bias=torch.zeros(8)),
                dict(bias=torch.zeros(7, dtype=torch.float64)), dict(out=torch.zeros(4, 7, dtype=torch.float16)),
                dict(out=torch.zeros(3, 7))):
        with pytest.raises(ValueError):
            ops.penalize_rows(**dict(good, **bad))
    with pytest.raises(RuntimeError):
        ops.penalize_rows(**dict(good, logits=case.logits.double()))
    out = torch.full((4, 9), 5.0)
    assert ops.penalize_rows(**dict(good, out=out[:, :7])) is not None and bool((out[:, 7:] == 5.0).all())


# ------------------------------------------------------------------ Penalties ---
def test_penalties_object():
    p = kv_cache.Penalties()
    assert (p.repetition, p.presence, p.frequency, p.min_p, p.logit_bias, p.banned) == (1.0, 0.0, 0.0, 0.0, None, ())
    assert p.bias_row(5, "cpu") is None and p.floor_gap(1.0) is None
    with pytest.raises(AttributeError):
        p.repetition = 2.0
    inf, nan = float("inf"), float("nan")
    for bad in (dict(repetition=0.0), dict(repetition=-1.0), dict(repetition=nan), dict(repetition=inf), dict(presence=nan),
                dict(frequency=inf), dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=nan), dict(logit_bias=[1.0]),
                dict(logit_bias={-1: 1.0}), dict(logit_bias={1: nan}), dict(logit_bias={1: inf}),
                dict(logit_bias=torch.zeros(2, 3)), dict(logit_bias=torch.tensor([nan])), dict(banned=(-1,))):
        with pytest.raises(ValueError):
            kv_cache.Penalties(**bad)
    p = kv_cache.Penalties(1.1, 0.2, 0.3, 0.05, {1: 0.5, 3: -inf}, banned=[4, 2, 4])
    assert p.banned == (2, 4) and "Penalties(" in repr(p)
    assert p.bias_row(6, "cpu").tolist() == [0.0, 0.5, -inf, -inf, -inf, 0.0]
    with pytest.raises(ValueError, match="vocabulary"):
        p.bias_row(4, "cpu")
    with pytest.raises(ValueError, match="no token"):
        kv_cache.Penalties(banned=(0, 1)).bias_row(2, "cpu")
    t = kv_cache.Penalties(logit_bias=torch.tensor([1.0, 2.0, 3.0]), banned=(0,))
    assert t.bias_row(3, "cpu").tolist() == [-inf, 2.0, 3.0]
    with pytest.raises(ValueError):
        t.bias_row(4, "cpu")
    # floor_gap = fp32(T ln(min_p)), computed in double; off at T <= 0
    want = torch.tensor(0.7 * math.log(0.05), dtype=torch.float64).float().item()
    assert p.floor_gap(0.7) == want and want < 0 and p.floor_gap(0.0) is None and p.floor_gap(-1.0) is None


# ------------------------------------------------------------------ the loops ---
def _generate(kind, model, prompts, n, **kw):
    if kind == "ragged":
        return kv_cache.generate_ragged(model, prompts, n, **kw)
    return kv_cache.generate_paged(model, prompts, n, page_size=32, **kw)


def test_penalties_value_errors(monkeypatch):
    S.stub_steps(monkeypatch)
    model, prompts, pen, smp = S.Model(), S.prompts(3, 5), kv_cache.Penalties(frequency=1.0), kv_cache.Sampler(0)
    for kind in ("ragged", "paged"):
        with pytest.raises(ValueError, match="sampler"):
            _generate(kind, model, prompts, 4, penalties=pen)
        with pytest.raises(ValueError, match="Penalties"):
            _generate(kind, model, prompts, 4, sampler=smp, penalties=dict(frequency=1.0))
        with pytest.raises(ValueError, match="graph=True"):
            _generate(kind, model, prompts, 4, sampler=smp, penalties=pen, speculate=kv_cache.Speculation(graph=True))
        with pytest.raises(ValueError, match="vocabulary"):
            _generate(kind, model, prompts, 4, sampler=smp, penalties=kv_cache.Penalties(banned=(S.VOCAB,)))
    with pytest.raises(ValueError, match="sampler"):
        kv_cache.cached_generate(model, torch.zeros(1, 3, dtype=torch.long), 2, penalties=pen)
    with pytest.raises(ValueError, match="sampler"):
        kv_cache.naive_generate(model, torch.zeros(1, 3, dtype=torch.long), 2, None, pen)


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_banned_tokens_are_never_emitted_and_a_large_frequency_penalty_makes_tokens_distinct(kind, monkeypatch):
    table = S.stub_steps(monkeypatch)
    model, prompts, n = S.Model(), S.prompts(3, 9, 5), 20
    smp = kv_cache.Sampler(0.9, 0, 1.0, seed=4)
    bare = _generate(kind, model, prompts, n, sampler=smp)
    banned = tuple(sorted({int(t) for o, p in zip(bare, prompts) for t in o[len(p):]}))[:4]      # tokens it does emit
    got = _generate(kind, model, prompts, n, sampler=smp, penalties=kv_cache.Penalties(banned=banned))
    assert all(len(o) == len(p) + n and not set(o[len(p):].tolist()) & set(banned) for o, p in zip(got, prompts))
    # frequency above the logit range: a token is not drawn again while another is left
    spread = float(table.max() - table.min()) + 1.0
    pen = kv_cache.Penalties(frequency=4 * spread + 100.0)
    for sampler in (smp, kv_cache.Sampler(temperature=0)):
        got = _generate(kind, model, prompts, n, sampler=sampler, penalties=pen)
        for o, p in zip(got, prompts):
            first = o[len(p):len(p) + min(S.VOCAB, n)].tolist()
            assert len(set(first)) == len(first) == min(S.VOCAB, n)
    if kind == "paged":                                        # one history row per sample, gen_start its prompt's length
        pairs = kv_cache.generate_paged(model, prompts, n, page_size=32, sampler=smp, penalties=pen, n_samples=2)
        for b, prompt in enumerate(prompts):
            for j in range(2):
                alone = kv_cache.generate_paged(model, [prompt], n, page_size=32, sampler=smp, penalties=pen,
                                                streams=[2 * b + j])[0]
                assert torch.equal(alone, pairs[b][j])


PENALTIES = {"repetition": dict(repetition=1.6), "counts": dict(presence=0.8, frequency=1.2),
             "all": dict(repetition=1.4, presence=0.5, frequency=0.9, min_p=0.05, banned=(2,), logit_bias={3: 0.75, 5: -1.0})}
SAMPLERS = {"greedy": dict(temperature=0.0), "filtered": dict(temperature=0.9, top_k=5, top_p=0.95, seed=4)}
# name: (prompt lengths, new tokens, eos_id, k); block_size is 64
CASES = {"plain": ((3, 9, 5), 12, None, 3), "eos_mid_round": ((3, 9, 5), 20, 4, 3), "k7": ((6, 2, 11, 4), 23, None, 7),
         "up_to_block_size": ((50, 41, 57), 7, None, 3)}


@pytest.mark.parametrize("kind", ["ragged", "paged"])
@pytest.mark.parametrize("penalty", sorted(PENALTIES))
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_speculative_tokens_are_the_plain_loops_under_penalties(case, sampler, penalty, kind, monkeypatch):
    S.stub_steps(monkeypatch)
    lens, n, eos, k = CASES[case]
    model, prompts, smp = S.Model(), S.prompts(*lens), kv_cache.Sampler(**SAMPLERS[sampler])
    pen = kv_cache.Penalties(**PENALTIES[penalty])
    bare = _generate(kind, model, prompts, n, sampler=smp, eos_id=eos)
    plain = _generate(kind, model, prompts, n, sampler=smp, eos_id=eos, penalties=pen)
    # the penalties change the ranking here: ignoring them gives other tokens.  (Not asked of the one combination
    # in which they cannot: repetition alone scales every logit of a prompt that holds the whole vocabulary by
    # one monotone map, which leaves a greedy ranking as it was.)
    monotone = (penalty == "repetition" and sampler == "greedy"
                and all(len(set(p.tolist())) == S.VOCAB for p in prompts))
    assert monotone or any(not torch.equal(a, b) for a, b in zip(plain, bare))
    # an oracle drafter with the miss walking through every index 0 .. k (k: all accepted), one that is always
    # right, one that drafts the unpenalised run (wrong wherever the penalties matter), and the n-gram lookup
    drafters = [S.OracleDrafter(plain, S.VOCAB, lambda r, b: (r + b) % (k + 1)),
                S.OracleDrafter(plain, S.VOCAB, lambda r, b: None),
                S.OracleDrafter(bare, S.VOCAB, lambda r, b: None), None]
    accepted = set()
    for drafter in drafters:
        spec = kv_cache.Speculation(k=k, drafter=drafter)
        real = ops.spec_accept_draft

        def spy(*a, **kw):
            res = real(*a, **kw)
            accepted.update(m - 1 for m in res[:, 0].tolist() if m)
            return res

        monkeypatch.setattr(ops, "spec_accept_draft", spy)
        got = _generate(kind, model, prompts, n, sampler=smp, eos_id=eos, penalties=pen, speculate=spec)
        monkeypatch.setattr(ops, "spec_accept_draft", real)
        assert len(got) == len(plain)
        for g, w, p in zip(got, plain, prompts):
            assert g.dtype == w.dtype and g.device == p.device and torch.equal(g, w)
        assert spec.stats["emitted"] == sum(len(o) - len(p) for o, p in zip(plain, prompts))
    if n > k + 1 and eos is None:
        assert accepted >= set(range(k + 1)), accepted        # every acceptance count 0 .. k occurred
