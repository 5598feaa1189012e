"""GPU checks of the row sampler (``ops.sample_rows`` / ``dta_sample_rows``) against the fp64 oracle of
the definition (tests/_sample_oracle.py, computed on the CPU from the fp32-converted logits), its
bitwise batch invariance, and the ``sampler`` argument of the generate loops end to end.

Acceptance (``_sample_oracle.check_row``): degenerate, greedy, top-k 1, one-hot and V = 1 rows match
token for token; otherwise the token must be kept by the oracle and ``u Z`` must lie within E of its
CDF step, E = 2^-23 (sum_kept w_i (|z_i| + 8) + D(V) Z), and the logprob within E / Z + 2^-20.  Every
top-p input keeps a margin of 16 E from the masses it is compared with, asserted on the CPU for every
row: the midpoint construction, or -- for p = 0.9 -- rows whose two largest logits are raised so far
above the rest (1.5 (ln V + 5)) that 0.9 falls between the mass of the first and of both, whatever
the temperature in [0.7, 1.5]."""
import math

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _poison
import _sample_oracle as orc
from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import Ndiff_transformer as ND
from differential_transformer_replication_amd import control as C
from differential_transformer_replication_amd import kv_cache, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = [1, 7, 255, 256, 257, 4099, 12000, 50257]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
TEMPS, PS = [0.0, 0.7, 1.0, 1.5], [1.0, 0.9, "mid"]


def _rows(seed, R, V, dtype):
    """randn * 4 rounded to ``dtype`` (bf16 at V = 12000: many ties), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * 4).to(dtype)


def _boosted(x):
    """The rows with their two largest logits raised for the p = 0.9 cases (module docstring)."""
    x = x.clone()
    V = x.shape[1]
    if V < 2:
        return x
    top = x.float().topk(2, dim=1)
    rest = x.float().topk(min(3, V), dim=1).values[:, -1] if V > 2 else top.values[:, 1]
    lift = rest + 1.5 * (math.log(V) + 5)
    x[torch.arange(x.shape[0]), top.indices[:, 0]] = lift.to(x.dtype)
    x[torch.arange(x.shape[0]), top.indices[:, 1]] = (lift - 0.5).to(x.dtype)
    return x


def _mid(x_row, T, k):
    """A midpoint top-p for one row: between its kept distinct values, after up to 3 of them."""
    if not T > 0:
        return 0.5
    row = orc.Row(x_row, T, k, 1.0)
    if row.degenerate:
        return 0.5
    classes = len(np.unique(np.asarray(x_row, dtype=np.float32)[row.kept]))
    return orc.midpoint_p(x_row, T, k, min(3, classes - 1)) if classes >= 2 else 0.5


def _check(x_cpu, T, k, p, seed, stream, offset, tok, lp):
    """Every row of a launch against the oracle; T, k, p scalars or per-row lists."""
    tok, lp = tok.cpu(), lp.cpu()
    R, V = x_cpu.shape
    assert tok.dtype == torch.int64 and tok.shape == (R,) and bool(((tok >= -1) & (tok < V)).all())
    xf = x_cpu.float().numpy()
    at = lambda v, r: v[r] if isinstance(v, (list, tuple)) else v       # noqa: E731
    for r in range(R):
        orc.check_row(xf[r], at(T, r), at(k, r), at(p, r), seed, at(stream, r), at(offset, r), tok[r], lp[r].item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("V", VS)
def test_scalar_parameters(V, dtype):
    R = 3
    base = _rows(1000 + V, R, V, dtype)
    lifted = _boosted(base)
    dev = {id(base): base.to(DEV), id(lifted): lifted.to(DEV)}
    strm = torch.tensor([5, 2 ** 40 + 1, -3], device=DEV)
    off = torch.tensor([0, 9, 2 ** 33], device=DEV)
    runs = []                                                       # (rows, row slice, T, k, p, tok, lp): one sync at the end
    for T in TEMPS:
        for k in (0, 1, 50, V):
            for p in PS:
                x = lifted if p == 0.9 else base
                parts = [slice(0, R)] if p != "mid" else [slice(r, r + 1) for r in range(R)]   # a scalar midpoint is one row's
                for s in parts:
                    pv = _mid(x[s.start].float().numpy(), T, k) if p == "mid" else p
                    tok, lp = ops.sample_rows(dev[id(x)][s], T, k, pv, seed=77, stream=strm[s], offset=off[s],
                                              return_logprobs=True)
                    runs.append((x, s, T, k, p, pv, tok, lp))
    torch.cuda.synchronize()
    for x, s, T, k, p, pv, tok, lp in runs:
        _check(x[s], T, k, pv, 77, strm[s].tolist(), off[s].tolist(), tok, lp)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("V", [7, 257, 12000, 50257])
def test_per_row_parameters_in_one_launch(V, dtype):
    R = 64
    base = _rows(2000 + V, R, V, dtype)
    lifted = _boosted(base)
    Ts = [TEMPS[r % 4] for r in range(R)]
    ks = [(0, 1, 50, V)[(r // 4) % 4] for r in range(R)]
    kinds = [PS[(r // 16) % 3] for r in range(R)]
    x = torch.stack([lifted[r] if kinds[r] == 0.9 else base[r] for r in range(R)])
    nan = float("nan")
    ps = [_mid(x[r].float().numpy(), Ts[r], ks[r]) if kinds[r] == "mid" else kinds[r] for r in range(R)]
    Ts[48], ps[49], ks[50], ks[51] = nan, nan, -4, V + 9            # NaN T: greedy; NaN p, k <= 0, k > V: off
    strm = [(r * 2654435761) % (2 ** 62) for r in range(R)]
    off = [r % 5 for r in range(R)]
    tok, lp = ops.sample_rows(x.to(DEV), torch.tensor(Ts, device=DEV), torch.tensor(ks, device=DEV),
                              torch.tensor(ps, device=DEV), seed=2 ** 63 + 11, stream=torch.tensor(strm, device=DEV),
                              offset=torch.tensor(off, device=DEV), return_logprobs=True)
    Ts[48], ps[49] = 0.0, 1.0
    _check(x, Ts, ks, ps, 2 ** 63 + 11, strm, off, tok, lp)
    # defaults: stream = the row index, offset = 0, no logprobs
    tok, lp = ops.sample_rows(x.to(DEV), seed=3, return_logprobs=True)
    _check(x, 1.0, 0, 1.0, 3, list(range(R)), [0] * R, tok, lp)
    assert torch.equal(ops.sample_rows(x.to(DEV), seed=3), tok)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_exact_rows(dtype):
    """Rows whose token is fixed by the definition: degenerate, one-hot, V = 1, top-k 1, greedy with ties."""
    ninf, inf, nan = float("-inf"), float("inf"), float("nan")
    for V in (1, 9, 300, 16000):
        x = _rows(3000 + V, 8, V, dtype)
        x[1, V // 2] = nan
        x[2, V - 1] = inf
        x[3, :] = ninf
        x[4, :] = ninf
        x[4, V // 3] = -2.0                                         # one-hot
        x[5, :] = 1.25                                              # all equal: greedy takes index 0
        x[6, 0] = ninf if V > 1 else 0.0
        x[7, -1] = x[7].float().max().item() + 1.0                  # the maximum in the last column
        want_greedy = [int(np.flatnonzero(r == r.max())[0]) for r in x.float().numpy()[[0, 4, 5, 6, 7]]]
        for T, k in ((0.0, 0), (1.0, 1), (0.7, 1), (-1.0, 5)):
            tok, lp = ops.sample_rows(x.to(DEV), T, k, 1.0, seed=9, return_logprobs=True)
            tok, lp = tok.cpu(), lp.cpu()
            assert tok[[1, 2, 3]].tolist() == [-1, -1, -1] and bool(torch.isnan(lp[[1, 2, 3]]).all())
            assert tok[4] == V // 3 and lp[4] == 0.0
            assert tok[7] == V - 1                                  # a single maximum: greedy and top-1 take it
            if not T > 0:
                assert tok[[0, 4, 5, 6, 7]].tolist() == want_greedy
            _check(x, T, k, 1.0, 9, list(range(8)), [0] * 8, tok, lp)
        # -0 and +0 compare equal: the lowest index wins
        z = torch.zeros(2, V, dtype=dtype)
        z[0, 0::2] = -0.0
        assert ops.sample_rows(z.to(DEV), 0.0).tolist() == [0, 0]


def test_a_strided_view_between_guard_bands():
    for dtype, V, stride in ((torch.bfloat16, 4099, 4101), (torch.float32, 257, 259), (torch.float16, 12000, 12003),
                             (torch.bfloat16, 50257, 50264)):
        R = 3
        x = _rows(4000 + V, R, V, dtype)
        with _poison.poisoned_allocations() as session:
            arena = _poison.Arena(((R - 1) * stride + V + 5) * dtype.itemsize, DEV, "logits")
            view = arena.view(dtype, (R, V), (stride, 1), offset=3)          # an odd offset: no row is 16-byte aligned
            view.copy_(x.to(DEV))
            assert view.data_ptr() % 16 != 0
            tok, lp = ops.sample_rows(view, 0.8, 50, 1.0, seed=6, return_logprobs=True)
            session.check()
            arena.check()
            session.assert_results_finite(["tokens", "logprobs"])
        _check(x, 0.8, 50, 1.0, 6, [0, 1, 2], [0, 0, 0], tok, lp)
        # the same rows, packed and aligned: the same bits
        tok2, lp2 = ops.sample_rows(x.to(DEV), 0.8, 50, 1.0, seed=6, return_logprobs=True)
        assert torch.equal(tok, tok2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


@pytest.mark.parametrize("V,dtype", [(12000, torch.bfloat16), (50257, torch.bfloat16), (4099, torch.float32),
                                     (255, torch.float16)])
def test_batch_invariance_is_bitwise(V, dtype):
    x8 = _boosted(_rows(5000 + V, 8, V, dtype)).to(DEV)
    others = _rows(5001 + V, 64, V, dtype).to(DEV)
    T = torch.tensor([0.7, 1.0, 1.5, 0.0, 0.9, 1.0, 0.7, 1.3], device=DEV)
    k = torch.tensor([0, 50, 1, 0, V, 50, 7, 0], dtype=torch.int32, device=DEV)
    p = torch.tensor([0.9, 0.9, 1.0, 0.5, 1.0, 0.37, 0.9, 0.613], device=DEV)
    strm = torch.tensor([11, 12, 13, 14, 15, 2 ** 50, 17, 18], device=DEV)
    off = torch.tensor([0, 1, 2, 3, 4, 5, 2 ** 35, 7], device=DEV)
    bits = lambda t: t.view(torch.int32)                                # noqa: E731

    tok, lp = ops.sample_rows(x8, T, k, p, seed=123, stream=strm, offset=off, return_logprobs=True)
    tok_b, lp_b = ops.sample_rows(x8, T, k, p, seed=123, stream=strm, offset=off, return_logprobs=True)
    assert torch.equal(tok, tok_b) and torch.equal(bits(lp), bits(lp_b))            # the same launch twice
    assert bool((tok >= 0).all())
    for r in range(8):                                                              # eight launches of one row
        s = slice(r, r + 1)
        t1, l1 = ops.sample_rows(x8[s], T[s], k[s], p[s], seed=123, stream=strm[s], offset=off[s], return_logprobs=True)
        assert torch.equal(t1, tok[s]) and torch.equal(bits(l1), bits(lp[s])), r
    where = torch.tensor([63, 5, 40, 0, 17, 33, 62, 8], device=DEV)                 # permuted among other rows
    big = others.clone()
    big[where] = x8
    full = lambda v, fill: torch.full((64,), fill, dtype=v.dtype, device=DEV).index_copy_(0, where, v)   # noqa: E731
    t64, l64 = ops.sample_rows(big, full(T, 1.1), full(k, 3), full(p, 0.8), seed=123, stream=full(strm, 99),
                               offset=full(off, 1), return_logprobs=True)
    assert torch.equal(t64[where], tok) and torch.equal(bits(l64[where]), bits(lp))
    other_seed = ops.sample_rows(x8, T, k, p, seed=124, stream=strm, offset=off)
    other_off = ops.sample_rows(x8, T, k, p, seed=123, stream=strm, offset=off + 1)
    draws = torch.tensor([0, 1, 4, 5, 6, 7], device=DEV)                            # rows 2, 3: top-1 and greedy
    assert torch.equal(other_seed[[2, 3]], tok[[2, 3]]) and torch.equal(other_off[[2, 3]], tok[[2, 3]])
    assert not (torch.equal(other_seed[draws], tok[draws]) and torch.equal(other_off[draws], tok[draws]))


# -------------------------------------------------------------- end to end ---
BS, P, VOCAB = 128, 32, 97
FP8 = "fp8_e4m3"


def _model(which):
    if which == "diff":
        torch.manual_seed(0)
        model = D.DiffTransformer(vocab_size=VOCAB, n_embd=256, n_head=2, n_layer=2, block_size=BS, dropout=0.0)
    elif which == "alt3":
        torch.manual_seed(1)
        model = ND.AlternatingDiffTransformer(VOCAB, 256, 2, 2, BS, 0.0, n_terms=3)
    else:
        torch.manual_seed(2)
        model = C.StandardTransformer(VOCAB, 256, 4, 2, BS, 0.0)
    model = model.to(DEV).eval()
    for p in model.parameters():
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model.to(torch.bfloat16)


def _hand_loop(model, prompts, n, pick, **flags):
    """``generate_paged``'s loop by hand over ``prefill_paged`` / ``decode_paged`` with ``pick(logits)`` as the sampler."""
    cache = kv_cache.PagedKVCache(16, P, max_seqs=len(prompts), **flags)
    seqs, logits = kv_cache.prefill_paged(model, prompts, cache)
    toks = []
    for step in range(n):
        toks.append(pick(logits))
        if step + 1 < n:
            logits = kv_cache.decode_paged(model, seqs, toks[-1], cache)
    toks = torch.cat(toks, dim=1)
    return [torch.cat([p, toks[b]]) for b, p in enumerate(prompts)]


@pytest.mark.parametrize("fast", [False, True], ids=["eager", "graph_fused"])
@pytest.mark.parametrize("kv_dtype", [None, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_generate_paged_with_a_sampler(which, kv_dtype, fast):
    model = _model(which)
    g = torch.Generator().manual_seed(8)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n in (12, 3, 31)]
    flags = dict(kv_dtype=kv_dtype, graph=fast, fused_step=fast)
    n = 12
    same = lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))   # noqa: E731
    s = kv_cache.Sampler(0.8, 50, 0.9, seed=1)
    with torch.no_grad():
        one = kv_cache.generate_paged(model, prompts, n, page_size=P, sampler=s, **flags)
        two = kv_cache.generate_paged(model, prompts, n, page_size=P, sampler=s, **flags)
        assert same(one, two) and all(len(o) == len(p) + n for o, p in zip(one, prompts))
        assert all(int(o.min()) >= 0 and int(o.max()) < VOCAB for o in one)
        pairs = kv_cache.generate_paged(model, prompts, n, page_size=P, sampler=s, n_samples=2, **flags)
        assert all(len(pr) == 2 for pr in pairs) and any(not torch.equal(a, b) for a, b in pairs)
        # temperature 0: the argmax loop over decode_paged
        greedy = kv_cache.generate_paged(model, prompts, n, page_size=P, sampler=kv_cache.Sampler(temperature=0), **flags)
        assert same(greedy, _hand_loop(model, prompts, n, lambda lg: lg.argmax(dim=-1, keepdim=True), **flags))
        # no sampler: the reference's softmax + multinomial, token for token
        torch.manual_seed(31)
        plain = kv_cache.generate_paged(model, prompts, n, page_size=P, sampler=None, **flags)
        torch.manual_seed(31)
        want = _hand_loop(model, prompts, n, lambda lg: torch.multinomial(F.softmax(lg, dim=-1), num_samples=1), **flags)
        assert same(plain, want)


@pytest.mark.parametrize("which", ["diff", "alt3", "ctrl"])
def test_model_generate_and_generate_ragged_with_a_sampler(which, monkeypatch):
    model = _model(which)
    idx = torch.randint(0, VOCAB, (2, 9), generator=torch.Generator().manual_seed(4)).to(DEV)
    s = kv_cache.Sampler(0.9, 20, 0.95, seed=5)
    with torch.no_grad():
        a, b = model.generate(idx, 6, sampler=s), model.generate(idx, 6, sampler=s)
        assert torch.equal(a, b) and a.shape == (2, 15) and torch.equal(a[:, :9], idx)
        g = model.generate(idx, 6, sampler=kv_cache.Sampler(temperature=0))
        logits = model(g[:, :-1])[0][:, 8:, :]                      # greedy: every new token is its row's argmax
        top2 = logits.float().topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 0.1                 # where the full forward cannot flip the cached step's argmax
        assert torch.equal(g[:, 9:][clear], logits.argmax(dim=-1)[clear])
        monkeypatch.setenv("DTA_KV_CACHE", "0")                     # the naive loop takes the sampler too
        c, d = model.generate(idx, 4, sampler=s), model.generate(idx, 4, sampler=s)
        assert torch.equal(c, d) and c.shape == (2, 13)
        monkeypatch.delenv("DTA_KV_CACHE")
        prompts = [idx[0, :5], idx[1]]
        r1 = kv_cache.generate_ragged(model, prompts, 6, sampler=s)
        r2 = kv_cache.generate_ragged(model, prompts, 6, sampler=s, graph=True, fused_step=True)
        assert all(torch.equal(x, y) for x, y in zip(r1, r2))
