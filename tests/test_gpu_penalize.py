"""GPU checks of the penalty row kernel (``ops.penalize_rows`` / ``dta_penalize_rows``): bit for bit against
``ops.penalize_rows_reference`` run on the CPU (itself held to the pure-Python definition by
tests/test_penalize_cpu.py) at every vocabulary band, dtype and layout, with poisoned outputs, workspace and
guard bands; its row independence; and the ``penalties`` argument of the generate loops on a real model, where
speculative rounds must emit the plain loop's tokens."""
import pytest
import torch

import _penalty as P
import _poison
import _spec as S
from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import kv_cache, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
LDS_MAX = ops.PENALTY_LDS_MAX_V
VS = [1, 7, 2048, 2049, 12000, 40000, LDS_MAX, LDS_MAX + 1]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _dirty_workspaces():
    for ws in ops._PENALTY_WS.values():
        ws.fill_(0xA5)


def _run(case, device=DEV, **kw):
    return ops.penalize_rows(**case.args(device, **kw))


def _want(case, **kw):
    """The reference on the CPU, from the logits as the device converts them to fp32: exact for every value
    that is not a NaN, and a 16-bit NaN gets the payload the hardware conversion gives it (torch's CPU
    conversion of an fp16 NaN gives another), so "a NaN is written through" is checked on those bits."""
    a = case.args("cpu", **kw)
    a["logits"] = case.logits.to(DEV).float().cpu()
    return ops.penalize_rows_reference(**a)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("V", VS)
def test_kernel_is_the_reference_bit_for_bit(V, dtype):
    assert ops.penalize_rows_supported()
    assert (ops._lib.load().dta_penalize_rows_workspace_bytes(5, V) == 0) == (V <= LDS_MAX)
    runs = []
    for B, Tn, draft in ((1, 1, False), (5, 1, False), (2, 4, True)):
        case = P.Case(B, Tn, V, dtype, seed=V + 10 * B, draft=draft)
        for name, kw in case.features().items():
            _dirty_workspaces()
            with _poison.poisoned_allocations() as session:
                got = _run(case, **kw)
                session.check()
            runs.append((B, Tn, name, got, _want(case, **kw), case))
    made = 0
    for B, Tn, name, got, want, case in runs:
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert P.same_but_made_nans(got, want, case.logits), (B, Tn, name, P.first_diff(got, want))
        made += int(P.made_nans(want, case.logits).sum())
        if V > 2:
            # the one NaN of the inputs, converted by the kernel itself: float(bf16 / f16 / f32 quiet NaN), fixed bits
            assert int(got.view(torch.int32)[(B * Tn) // 2, 1]) == 0x7FC00000, (B, Tn, name)
    assert (made > 0) == (V > 2)                                # +inf on a banned column: a NaN the arithmetic makes
    runs = [r[:5] for r in runs]
    # the features do something here: their outputs differ from the unpenalised row's
    plain = {(B, Tn): want for B, Tn, name, _, want in runs if name == "none"}
    if V >= 7:
        for B, Tn, name, _, want in runs:
            if name != "none" and B > 1:
                assert not P.same_bits(want, plain[(B, Tn)]), name


@pytest.mark.parametrize("V,dtype,stride,out_stride", [(12000, torch.bfloat16, 12003, 12001), (257, torch.float16, 259, 300),
                                                       (LDS_MAX + 1, torch.float32, LDS_MAX + 2, LDS_MAX + 4),
                                                       (7, torch.float32, 9, 7)])
def test_strided_views_between_guard_bands(V, dtype, stride, out_stride):
    B, Tn = 2, 4
    R = B * Tn
    case = P.Case(B, Tn, V, dtype, seed=77)
    kw = case.features()["all"]
    want = _want(case, **kw)
    _dirty_workspaces()
    with _poison.poisoned_allocations() as session:
        xin = _poison.Arena(((R - 1) * stride + V + 5) * dtype.itemsize, DEV, "logits")
        view = xin.view(dtype, (R, V), (stride, 1), offset=3)                  # an odd offset: no row is vector aligned
        view.copy_(case.logits.to(DEV))
        xout = _poison.Arena(((R - 1) * out_stride + V + 3) * 4, DEV, "out")
        out = xout.view(torch.float32, (R, V), (out_stride, 1), offset=1)
        hist = _poison.Arena((B * (case.cap + 3)) * 4, DEV, "hist").view(torch.int32, (B, case.cap), (case.cap + 3, 1), 1)
        hist.copy_(case.hist.to(DEV))
        a = case.args(DEV, **kw)
        a.update(logits=view, hist=hist, out=out)
        got = ops.penalize_rows(**a)
        session.check()
        xin.check()
        xout.check()
        assert torch.equal(view.cpu().view(torch.int16 if dtype.itemsize == 2 else torch.int32),
                           case.logits.view(torch.int16 if dtype.itemsize == 2 else torch.int32))
    assert got is out and P.same_but_made_nans(out, want, case.logits), P.first_diff(out, want)
    assert P.same_bits(_run(case, **kw), out)                                   # packed and aligned: the same bits


@pytest.mark.parametrize("V,dtype", [(12000, torch.bfloat16), (LDS_MAX + 1, torch.float32), (7, torch.float16)])
def test_long_histories(V, dtype):
    """cap = 4352: histories of length 0 and 1, one full of one token, one full of distinct tokens."""
    cap, B = 4352, 4
    case = P.Case(B, 1, V, dtype, cap=cap, seed=5, draft=False)
    case.hist = torch.stack([torch.zeros(cap, dtype=torch.int32), torch.full((cap,), V - 1, dtype=torch.int32),
                             torch.full((cap,), min(3, V - 1), dtype=torch.int32),
                             (torch.arange(cap, dtype=torch.int32) * 7) % V])
    case.hlen = P.i32([0, 1, cap, cap])
    case.gen_start = P.i32([0, 0, 100, 17])
    for name in ("rep", "freq", "all"):
        kw = case.features()[name]
        _dirty_workspaces()
        got, want = _run(case, **kw), _want(case, **kw)
        assert P.same_but_made_nans(got, want, case.logits), (name, P.first_diff(got, want))


@pytest.mark.parametrize("V,dtype", [(2049, torch.bfloat16), (LDS_MAX + 1, torch.bfloat16), (40000, torch.float32)])
def test_row_independence_is_bitwise(V, dtype):
    B, Tn = 8, 2
    case = P.Case(B, Tn, V, dtype, seed=21)
    kw = case.features()["per_seq"]
    a = case.args(DEV, **kw)
    full = ops.penalize_rows(**a).clone()
    _dirty_workspaces()
    assert P.same_bits(ops.penalize_rows(**a), full)                            # again, on a dirty workspace
    seq = lambda t, idx: t[idx] if isinstance(t, torch.Tensor) and t.shape[:1] == (B,) else t   # noqa: E731
    rows = lambda idx: (idx[:, None] * Tn + torch.arange(Tn, device=DEV)[None, :]).reshape(-1)  # noqa: E731
    for b in range(B):                                                          # eight launches of one sequence
        idx = torch.tensor([b], device=DEV)
        one = {k: seq(v, idx) for k, v in a.items()}
        one["logits"] = a["logits"][rows(idx)]
        assert P.same_bits(ops.penalize_rows(**one), full[rows(idx)]), b
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=DEV)                   # the sequences permuted
    shuffled = {k: seq(v, perm) for k, v in a.items()}
    shuffled["logits"] = a["logits"][rows(perm)]
    assert P.same_bits(ops.penalize_rows(**shuffled), full[rows(perm)])


def test_sampling_the_kernels_rows_is_sampling_the_references():
    case = P.Case(4, 2, 12000, torch.bfloat16, seed=9, specials=False)
    kw = case.features()["all"]
    got = _run(case, **kw)
    want = _want(case, **kw).to(DEV)
    off = torch.arange(8, device=DEV)
    a, la = ops.sample_rows(got, 0.8, 50, 0.9, seed=3, offset=off, return_logprobs=True)
    b, lb = ops.sample_rows(want, 0.8, 50, 0.9, seed=3, offset=off, return_logprobs=True)
    assert torch.equal(a, b) and P.same_bits(la, lb) and bool((a >= 0).all())


# ------------------------------------------------------------------ the loops ---
BS, VOCAB = 64, 97
PROMPT_LENS = [5, 17, 40]
PEN = dict(repetition=1.3, presence=0.2, frequency=0.4, banned=(3, 11), logit_bias={7: 0.5})


def _model():
    torch.manual_seed(0)
    model = D.DiffTransformer(vocab_size=VOCAB, n_embd=256, n_head=2, n_layer=2, block_size=BS, dropout=0.0).to(DEV).eval()
    for p in model.parameters():
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model


def _prompts():
    # of prompt seeds 1 .. 12 the one whose penalised plain loop has the widest smallest gap on both the
    # unquantised and the fp8 pool (4.0e-3 and 3.3e-3)
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n in PROMPT_LENS]


FLAGS = {"ragged": (kv_cache.generate_ragged, {}), "ragged_graph_fused": (kv_cache.generate_ragged, dict(graph=True, fused_step=True)),
         "paged": (kv_cache.generate_paged, dict(page_size=32)),
         "paged_graph_fused": (kv_cache.generate_paged, dict(page_size=32, graph=True, fused_step=True)),
         "paged_fp8": (kv_cache.generate_paged, dict(page_size=32, kv_dtype="fp8_e4m3")),
         "paged_fp8_graph_fused": (kv_cache.generate_paged, dict(page_size=32, kv_dtype="fp8_e4m3", graph=True, fused_step=True))}


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_real_model_speculation_emits_the_plain_loops_tokens(kind, monkeypatch):
    """The fp32 DiffTransformer of tests/test_gpu_spec.py (97 / 256 / 2 heads / 2 layers, block 64, prompts
    5 / 17 / 40, 20 new tokens, K = 3, temperature 0) with repetition, presence and frequency penalties, two
    banned tokens and a bias.  Measured on the plain loop alone: the smallest top-1 - top-2 gap g of the
    penalised rows it samples, asserted >= 1e-3; the speculative rounds' penalised rows on the accepted path must
    stay within g / 2 of them (a token can only flip at or above that), and the tokens are equal outright.  The
    penalties matter: the unpenalised loop emits other tokens, and no banned token is emitted.  Prints g and
    |dlogit| (measured: g = 4.006e-3 on the unquantised caches and 3.258e-3 on the fp8 pool, |dlogit| at most
    6.6e-7)."""
    gen, kw = FLAGS[kind]
    model, prompts = _model(), _prompts()
    B, n, k = len(prompts), 20, 3
    smp, pen = kv_cache.Sampler(temperature=0), kv_cache.Penalties(**PEN)
    seen, ms = [], []
    real, real_accept = ops.sample_rows, ops.spec_accept_draft

    def spy(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs=False):
        seen.append((logits.detach().float().reshape(B, -1, logits.shape[-1]).cpu(), offset.reshape(B, -1).cpu()))
        return real(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs)

    def spy_accept(*a, **kwa):
        res = real_accept(*a, **kwa)
        ms.append(res[:, 0].tolist())
        return res

    bare = gen(model, prompts, n, sampler=smp, **kw)
    monkeypatch.setattr(ops, "sample_rows", spy)
    plain = gen(model, prompts, n, sampler=smp, penalties=pen, **kw)
    assert any(not torch.equal(a, b) for a, b in zip(plain, bare))
    assert all(not bool(torch.isin(o[len(p):], torch.tensor(PEN["banned"], device=DEV)).any()) for o, p in zip(plain, prompts))
    plain_logits = torch.stack([s[0][:, 0] for s in seen])                      # (n, B, V), penalised
    top2 = plain_logits.topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"{kind}: smallest top-1 - top-2 gap of the penalised plain loop: {gap:.3e}")
    assert gap >= 1e-3, gap
    seen.clear()
    monkeypatch.setattr(ops, "spec_accept_draft", spy_accept)
    for drafter in (S.OracleDrafter([p.cpu() for p in plain], VOCAB, lambda r, b: (r + b) % (k + 1)), None):
        seen.clear()
        ms.clear()
        spec = kv_cache.Speculation(k=k, drafter=drafter)
        got = gen(model, prompts, n, sampler=smp, penalties=pen, speculate=spec, **kw)
        worst = 0.0
        for (logits, offset), m in zip(seen, ms):
            for b in range(B):
                for j in range(m[b]):                                           # the rows on the accepted path
                    d = logits[b, j] - plain_logits[int(offset[b, j]), b]
                    worst = max(worst, float(d[torch.isfinite(plain_logits[int(offset[b, j]), b])].abs().max()))
        print(f"{kind}: largest |dlogit| between the plain and the speculative path: {worst:.3e}, {spec.stats}")
        assert worst < gap / 2, (worst, gap)
        for a, b in zip(got, plain):
            assert torch.equal(a, b)
        assert spec.stats["emitted"] == B * n
        if drafter is not None:
            assert 0 < spec.stats["accepted"] < spec.stats["drafted"] and spec.stats["rounds"] < n - 1


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"], ids=["unquantised", "fp8"])
def test_each_of_two_samples_is_its_own_run(kv_dtype):
    model, prompts = _model(), _prompts()
    smp = kv_cache.Sampler(0.9, 5, 1.0, seed=6)
    pen = kv_cache.Penalties(repetition=1.2, frequency=0.3, min_p=0.05, banned=(3,))
    kw = dict(page_size=32, kv_dtype=kv_dtype, sampler=smp, penalties=pen)
    pairs = kv_cache.generate_paged(model, prompts, 12, n_samples=2, **kw)
    assert any(not torch.equal(a, b) for a, b in pairs)
    for b, prompt in enumerate(prompts):
        for j in range(2):
            alone = kv_cache.generate_paged(model, [prompt], 12, streams=[2 * b + j], **kw)[0]
            assert torch.equal(alone, pairs[b][j]), (b, j)


def test_model_generate_takes_penalties():
    model = _model()
    idx = torch.randint(0, VOCAB, (2, 9), generator=torch.Generator().manual_seed(4)).to(DEV)
    smp, pen = kv_cache.Sampler(0.9, 20, 0.95, seed=5), kv_cache.Penalties(frequency=50.0, banned=(0, 1, 2))
    out = model.generate(idx, 12, sampler=smp, penalties=pen)
    assert out.shape == (2, 21) and torch.equal(out[:, :9], idx) and torch.equal(out, model.generate(idx, 12, sampler=smp, penalties=pen))
    new = out[:, 9:]
    assert all(len(set(row.tolist())) == 12 for row in new) and int(new.min()) >= 3
