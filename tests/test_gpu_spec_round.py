"""GPU checks of the fixed-shape speculative round: ``dta_spec_feed_rows`` / ``dta_spec_commit_lengths`` against
their torch references bit for bit (every output, the whole of ``lengths``; edge rows and out-of-range device
values included), at a padded output stride, a row at a time, inside poisoned guard-banded buffers; and
``Speculation(graph=True)`` on the device: the stubbed loops (two calls of the model step however many rounds
ran), one real fp32 model on the ragged cache, and the paged cache on both kinds of pool with ``fused_step`` on
and off against the eager round."""
import pytest
import torch

import _poison as PZ
import _spec as S
import _spec_round as R
from conftest import rel_err
from differential_transformer_replication_amd import kv_cache, ops
from differential_transformer_replication_amd import diff_transformer as D

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _feed(st, K, **out):
    return ops.spec_feed_rows(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K, R.VOCAB, R.TOTAL, **out)


# ------------------------------------------------------------------ the kernels ---
@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("B", R.BATCHES)
def test_feed_kernel_is_the_reference(B, K):
    assert ops.spec_round_supported()
    for tag, st in R.states(B, K):
        want = ops.spec_feed_rows_reference(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K, R.VOCAB, R.TOTAL)
        dev = st.clone(DEV)
        got = _feed(dev, K)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (tag, B, K)
        for new, old in zip(dev.tensors(), st.tensors()):                          # the state is read only
            assert torch.equal(new.cpu(), old), tag
        # a padded row stride gives the packed outputs, and the padding is not written
        wide = torch.full((2, B, K + 6), -7, dtype=torch.int64, device=DEV)
        counts = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        _feed(dev, K, idx_out=wide[0, :, 3:K + 4], counts_out=counts, offset_out=wide[1, :, 3:K + 4])
        assert torch.equal(wide[0, :, 3:K + 4], got[0]) and torch.equal(wide[1, :, 3:K + 4], got[2])
        assert torch.equal(counts, got[1]) and int((wide == -7).sum()) == 2 * B * 5
        # a row's outputs are its outputs in a launch of its own
        for b in range(0, B, 7):
            one = S.State(*(t[b:b + 1].to(DEV).clone() for t in st.tensors()))
            for g, w in zip(_feed(one, K), got):
                assert torch.equal(g[0], w[b]), (tag, b)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("B", R.BATCHES)
def test_commit_kernel_is_the_reference(B, K, paged):
    lengths, result, slots = R.commit_inputs(B, K, 64, paged)
    want = ops.spec_commit_lengths_reference(lengths.clone(), result, K, 64, slots)
    mine, res, sl = lengths.to(DEV), result.to(DEV), None if slots is None else slots.to(DEV)
    assert ops.spec_commit_lengths(mine, res, K, 64, sl) is mine
    assert torch.equal(mine.cpu(), want)                                           # the whole of lengths
    assert torch.equal(res.cpu(), result) and (slots is None or torch.equal(sl.cpu(), slots))
    for b in range(0, B, 7):                                                       # a row in a launch of its own
        one = lengths.to(DEV)
        ops.spec_commit_lengths(one, res[b:b + 1].contiguous(), K, 64,
                                (torch.tensor([b], device=DEV) if slots is None else sl[b:b + 1].contiguous()))
        s = b if slots is None else int(slots[b].clamp(0, lengths.shape[0] - 1))
        assert int(one[s]) == int(want[s])
        one[s] = lengths[s]
        assert torch.equal(one.cpu(), lengths)


def test_what_is_not_written_keeps_its_poison():
    B, K, pad = 64, 3, 3
    for tag, st in R.states(B, K):
        dev = st.clone(DEV)
        arenas = [PZ.Arena(B * (K + 1 + pad) * 8, DEV, "idx_out"), PZ.Arena(B * 4 + 64, DEV, "counts_out"),
                  PZ.Arena(B * (K + 1 + pad) * 8, DEV, "offset_out")]
        idx = arenas[0].view(torch.int64, (B, K + 1), (K + 1 + pad, 1))
        counts = arenas[1].view(torch.int32, (B,), (1,))
        offset = arenas[2].view(torch.int64, (B, K + 1), (K + 1 + pad, 1))
        _feed(dev, K, idx_out=idx, counts_out=counts, offset_out=offset)
        torch.cuda.synchronize()
        for ar in arenas:
            ar.check()
        want = ops.spec_feed_rows_reference(st.hist, st.hlen, st.remaining, st.draft, st.dcnt, K, R.VOCAB, R.TOTAL)
        for g, w in zip((idx, counts, offset), want):
            assert torch.equal(g.cpu(), w), tag                                    # every entry written: no -1 left
        for new, old in zip(dev.tensors(), st.tensors()):
            assert torch.equal(new.cpu(), old), tag
    for paged in (False, True):
        lengths, result, slots = R.commit_inputs(B, K, 64, paged)
        n = lengths.shape[0]
        arena = PZ.Arena(n * 4 + 64, DEV, "lengths")
        mine = arena.view(torch.int32, (n,), (1,))
        mine.copy_(lengths)
        res, sl = result.to(DEV), None if slots is None else slots.to(DEV)
        ops.spec_commit_lengths(mine, res, K, 64, sl)
        torch.cuda.synchronize()
        arena.check()
        want = ops.spec_commit_lengths_reference(lengths.clone(), result, K, 64, slots)
        assert torch.equal(mine.cpu(), want)
        if paged:                                                                  # the slots nobody names
            named = set(slots.clamp(0, n - 1).tolist())
            assert all(int(mine[s]) == int(lengths[s]) for s in range(n) if s not in named) and len(named) == B
        assert torch.equal(res.cpu(), result) and (slots is None or torch.equal(sl.cpu(), slots))


# ------------------------------------------------------------------ the loops ---
def _count_steps(monkeypatch):
    """Wrap the two model-step names: calls[0] counts those that are not a prefill."""
    calls = [0]
    for name in ("_ragged_model_step", "_paged_model_step"):
        real = getattr(kv_cache, name)

        def step(*a, _real=real, _ragged=name == "_ragged_model_step", **kw):
            pos = a[3] if _ragged else a[4]
            calls[0] += pos is not None
            return _real(*a, **kw)

        monkeypatch.setattr(kv_cache, name, step)
    return calls


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_stubbed_loops_replay_one_graph(kind, monkeypatch):
    S.stub_steps(monkeypatch, DEV)
    calls = _count_steps(monkeypatch)
    model, k = S.Model(), 3
    prompts = [p.to(DEV) for p in S.prompts(28, 31, 5)]       # paged: 32-row pages, rounds cross a page boundary
    smp = kv_cache.Sampler(0.9, 5, 0.95, seed=4)
    gen = kv_cache.generate_ragged if kind == "ragged" else kv_cache.generate_paged
    kw = {} if kind == "ragged" else dict(page_size=32)
    monkeypatch.setattr(kv_cache, "PagedKVCache", S.RecordingPagedCache)
    for eos in (None, 4):
        plain = gen(model, prompts, 10, sampler=smp, eos_id=eos, **kw)
        plain_cache = S.RecordingPagedCache.last
        if kind == "paged":
            plain_cache.sync()
        cpu = [p.cpu() for p in plain]
        for miss in (lambda r, b: (r + b) % (k + 1), lambda r, b: 0, lambda r, b: None, "lookup"):
            stats = {}
            for graph in (False, True):
                drafter = None if miss == "lookup" else S.OracleDrafter(cpu, S.VOCAB, miss)
                spec = kv_cache.Speculation(k=k, drafter=drafter, graph=graph)
                calls[0] = 0
                got = gen(model, prompts, 10, sampler=smp, eos_id=eos, speculate=spec, **kw)
                for g, w in zip(got, plain):
                    assert g.device == w.device and g.dtype == w.dtype and torch.equal(g, w)
                stats[graph] = dict(spec.stats)
                if graph:                                     # warm-up and capture, however many rounds ran
                    assert calls[0] == 2 and spec.stats["rounds"] > 2
                else:
                    assert calls[0] == spec.stats["rounds"]
                if kind == "paged":
                    cache = S.RecordingPagedCache.last
                    assert cache.pages_in_use() == plain_cache.pages_in_use()
                    assert cache.host_lengths == plain_cache.host_lengths
                    assert cache.lengths[:3].tolist() == [cache.host_lengths[q] for q in range(3)]
            assert stats[True] == stats[False]


def test_a_library_without_the_symbols_is_an_error(monkeypatch):
    S.stub_steps(monkeypatch, DEV)
    monkeypatch.setattr(ops, "spec_round_supported", lambda: False)
    prompts = [p.to(DEV) for p in S.prompts(6, 3)]
    for gen in (kv_cache.generate_ragged, kv_cache.generate_paged):
        with pytest.raises(RuntimeError, match="dta_spec_feed_rows"):
            gen(S.Model(), prompts, 6, sampler=kv_cache.Sampler(0), speculate=kv_cache.Speculation(k=3, graph=True))


BS = 64
PROMPT_LENS = [5, 17, 40]


class _RecordingRagged(kv_cache.RaggedKVCache):
    last = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        _RecordingRagged.last = self


def _model():
    torch.manual_seed(0)
    model = D.DiffTransformer(vocab_size=97, n_embd=256, n_head=2, n_layer=2, block_size=BS, dropout=0.0).to(DEV).eval()
    for p in model.parameters():
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model


def test_real_model_ragged_tokens_logits_and_cache_rows(monkeypatch):
    """The fp32 DiffTransformer of ``test_gpu_spec.test_real_model_tokens_and_cache_rows`` (97 / 256 / 2 heads /
    2 layers, block 64, prompts 5 / 17 / 40, 24 new tokens, K = 3, temperature 0, oracle drafter with misses)
    with ``graph=True``.  Measured on the plain loop alone: its smallest top-1 - top-2 logit gap g, asserted
    >= 1e-3.  Then the largest |dlogit| between the plain path and the round's rows on the accepted path --
    the replayed rounds' rows are read from the graph's static logits after each replay; a round next to the
    window's end would take the eager path and be recorded by the same spy -- is asserted below g / 2 (a
    token can only flip at or above that),
    the tokens are equal, the device lengths are ``len(out) - 1`` and the cache rows below them match a fresh
    ``prefill_ragged`` to 1e-4.  Prints g and |dlogit| (measured: 7.477e-3 and 0, all 10 rounds replays)."""
    model = _model()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in PROMPT_LENS]
    B, n, k, smp = len(prompts), 24, 3, kv_cache.Sampler(temperature=0)
    seen, held, flag = [], {}, {"init": False, "replays": 0}
    real, real_accept = ops.sample_rows, ops.spec_accept_draft
    real_init, real_run = kv_cache.SpecRound.__init__, kv_cache.SpecRound.run

    def spy(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs=False):
        if flag["init"]:
            held["rows"] = logits                  # the capture's call is the last: the graph's static logits
        else:
            seen.append([logits.detach().float().reshape(B, -1, logits.shape[-1]).cpu(), offset.reshape(B, -1).cpu()])
        return real(logits, temperature, top_k, top_p, seed, stream, offset, return_logprobs)

    def spy_accept(*a, **kw):
        res = real_accept(*a, **kw)
        if not flag["init"]:
            seen[-1].append(res[:, 0].tolist())
        return res

    def init(self, *a, **kw):
        flag["init"] = True
        try:
            real_init(self, *a, **kw)
        finally:
            flag["init"] = False

    def run(self):
        real_run(self)
        flag["replays"] += 1
        seen.append([held["rows"].detach().float().reshape(B, -1, held["rows"].shape[-1]).cpu(), self.offset.cpu(),
                     self.result[:, 0].tolist()])

    monkeypatch.setattr(ops, "sample_rows", spy)
    plain = kv_cache.generate_ragged(model, prompts, n, sampler=smp)
    plain_logits = torch.stack([s[0][:, 0] for s in seen])                      # (n, B, V)
    top2 = plain_logits.topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"smallest top-1 - top-2 gap of the plain loop: {gap:.3e}")
    assert gap >= 1e-3, gap
    del seen[:]
    monkeypatch.setattr(ops, "spec_accept_draft", spy_accept)
    monkeypatch.setattr(kv_cache.SpecRound, "__init__", init)
    monkeypatch.setattr(kv_cache.SpecRound, "run", run)
    monkeypatch.setattr(kv_cache, "RaggedKVCache", _RecordingRagged)
    spec = kv_cache.Speculation(k=k, drafter=S.OracleDrafter([p.cpu() for p in plain], 97, lambda r, b: (r + b) % (k + 1)),
                                graph=True)
    got = kv_cache.generate_ragged(model, prompts, n, sampler=smp, speculate=spec)
    cache = _RecordingRagged.last
    worst = 0.0
    for logits, offset, m in seen:
        for b in range(B):
            for j in range(m[b]):                                               # the rows on the accepted path
                worst = max(worst, float((logits[b, j] - plain_logits[int(offset[b, j]), b]).abs().max()))
    print(f"largest |dlogit| between the plain path and the graph round: {worst:.3e} "
          f"({flag['replays']} replayed rounds of {spec.stats['rounds']})")
    assert len(seen) == spec.stats["rounds"] + 1 and flag["replays"] >= 3
    assert worst < gap / 2, (worst, gap)
    for a, b in zip(got, plain):
        assert torch.equal(a, b)
    st = spec.stats
    assert st["emitted"] == 3 * n and 0 < st["accepted"] < st["drafted"] and st["rounds"] < n - 1
    assert cache.lengths.tolist() == [len(o) - 1 for o in got]
    fresh = kv_cache.RaggedKVCache()
    with torch.no_grad():
        kv_cache.prefill_ragged(model, [o[:-1] for o in got], fresh)
    for layer, rows in fresh.rows.items():
        for b, o in enumerate(got):
            L = len(o) - 1
            assert rel_err(cache.rows[layer][b, :L], rows[b, :L]) <= 1e-4, (layer, b)


@pytest.mark.parametrize("fused_step", [False, True])
@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"])
def test_real_model_paged_is_the_eager_round(kv_dtype, fused_step, monkeypatch):
    """``generate_paged`` of the same fp32 model on the unquantised pool and on an fp8 pool, ``fused_step`` on and
    off: the graph round's tokens and pages are the eager round's (``Speculation(graph=False)``, same drafter,
    same pool).  32-row pages, the smallest the kernels have (``ops.PAGE_SIZES``): prompts of 28 / 31 / 5 / 20
    tokens and 20 new ones cross a page boundary in three sequences, and a rejected draft frees a page."""
    model = _model()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 97, (n,), generator=g).to(DEV) for n in (28, 31, 5, 20)]
    n, k, smp = 20, 3, kv_cache.Sampler(temperature=0)
    kw = dict(sampler=smp, page_size=32, kv_dtype=kv_dtype, fused_step=fused_step)
    plain = [p.cpu() for p in kv_cache.generate_paged(model, prompts, n, **kw)]
    monkeypatch.setattr(kv_cache, "PagedKVCache", S.RecordingPagedCache)
    freed = []
    real_trim = kv_cache.PagedKVCache._trim

    def trim(self, q):
        before = self.pages_in_use()
        real_trim(self, q)
        freed.append(before - self.pages_in_use())

    monkeypatch.setattr(S.RecordingPagedCache, "_trim", trim)
    outs = {}
    for graph in (False, True):
        spec = kv_cache.Speculation(k=k, drafter=S.OracleDrafter(plain, 97, lambda r, b: (r + b) % (k + 1)), graph=graph)
        del freed[:]
        got = kv_cache.generate_paged(model, prompts, n, speculate=spec, **kw)
        cache = S.RecordingPagedCache.last
        outs[graph] = (got, cache.pages_in_use(), dict(cache.host_lengths), dict(spec.stats))
        assert cache.lengths[:4].tolist() == [cache.host_lengths[q] for q in range(4)]
        assert any(f > 0 for f in freed), "no rejected draft freed a page"
    for a, b in zip(outs[True][0], outs[False][0]):
        assert torch.equal(a, b)
    assert outs[True][1:] == outs[False][1:]
    assert outs[True][3]["rounds"] >= 3
