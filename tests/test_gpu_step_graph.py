"""The graph-replayed one-token step of ``decode_ragged`` / ``decode_paged`` (``graph=True``,
``kv_cache.SeqDecodeGraph``), with and without the fused row write (``fused_step=True``).

Every case feeds a graph cache and an eager twin made with the flags off -- the step as it was
before either flag existed -- the same tokens; after every step the logits are bitwise equal
(``torch.equal``: no tolerance) and the device lengths are equal.  Tiny models of the three classes,
block_size 128, page size 32; 70 steps from prompts of 5, 30 and 17 tokens cross the page
boundaries at 32, 64 and 96."""
import pytest
import torch

from differential_transformer_replication_amd import diff_transformer as D
from differential_transformer_replication_amd import Ndiff_transformer as ND
from differential_transformer_replication_amd import control as C
from differential_transformer_replication_amd import kv_cache

pytestmark = pytest.mark.gpu
DEV = "cuda"
BS, P, POOL, VOCAB = 128, 32, 16, 97
FP8 = "fp8_e4m3"
LENS = [5, 30, 17]
WHICH = ["diff", "alt3", "ctrl"]


def _model(which, dtype=torch.float32):
    if which == "diff":
        torch.manual_seed(0)
        model = D.DiffTransformer(vocab_size=VOCAB, n_embd=256, n_head=2, n_layer=2, block_size=BS, dropout=0.0)
    elif which == "alt3":
        torch.manual_seed(1)
        model = ND.AlternatingDiffTransformer(VOCAB, 256, 2, 2, BS, 0.0, n_terms=3)
    else:
        torch.manual_seed(2)
        model = C.StandardTransformer(VOCAB, 256, 4, 2, BS, 0.0)        # N = 1, dv = hs = 64, RoPE
    model = model.to(DEV).eval()
    for p in model.parameters():          # non-zero lambdas so every branch weight differs
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    return model if dtype == torch.float32 else model.to(dtype)


def _prompts(seed, lens):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n in lens]


def _toks(g, B):
    return torch.randint(0, VOCAB, (B, 1), generator=g).to(DEV)


class _Ragged:
    """A graph cache and its flag-less twin on the ragged path, stepped together."""

    def __init__(self, model, prompts, fused):
        self.model = model
        self.caches = kv_cache.RaggedKVCache(graph=True, fused_step=fused), kv_cache.RaggedKVCache()
        with torch.no_grad():
            a, b = (kv_cache.prefill_ragged(model, prompts, c) for c in self.caches)
        assert torch.equal(a, b)

    def step(self, tok, active=None, tag=None):
        a, b = (kv_cache.decode_ragged(self.model, tok, c, active) for c in self.caches)
        assert torch.equal(a, b), tag
        assert torch.equal(self.caches[0].lengths, self.caches[1].lengths), tag
        return a


class _Paged:
    """The same on the paged path; both caches hand out the same sequence ids and slots."""

    def __init__(self, model, prompts, fused, kv_dtype=None, pool=POOL):
        self.model = model
        self.caches = (kv_cache.PagedKVCache(pool, P, kv_dtype=kv_dtype, graph=True, fused_step=fused),
                       kv_cache.PagedKVCache(pool, P, kv_dtype=kv_dtype))
        self.ids = self.prefill(prompts)

    def prefill(self, prompts):
        with torch.no_grad():
            (ia, a), (ib, b) = (kv_cache.prefill_paged(self.model, prompts, c) for c in self.caches)
        assert ia == ib and torch.equal(a, b)
        return ia

    def both(self, fn):
        out = [fn(c) for c in self.caches]
        assert out[0] == out[1]
        return out[0]

    def step(self, ids, tok, active=None, tag=None):
        a, b = (kv_cache.decode_paged(self.model, ids, tok, c, active) for c in self.caches)
        assert torch.equal(a, b), tag
        assert torch.equal(self.caches[0].lengths, self.caches[1].lengths), tag
        assert self.caches[0].pages == self.caches[1].pages, tag
        return a


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_decode_ragged_70_steps(which, fused):
    pair = _Ragged(_model(which), _prompts(3, LENS), fused)
    g = torch.Generator().manual_seed(4)
    for step in range(70):
        pair.step(_toks(g, 3), tag=(which, fused, step))
    assert pair.caches[0].lengths.tolist() == [75, 100, 87] and list(pair.caches[0].graphs) == [(3, False)]


@pytest.mark.parametrize("kv_dtype", [None, FP8])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_decode_paged_70_steps(which, fused, kv_dtype):
    pair = _Paged(_model(which), _prompts(3, LENS), fused, kv_dtype)
    g = torch.Generator().manual_seed(4)
    for step in range(70):
        pair.step(pair.ids, _toks(g, 3), tag=(which, fused, kv_dtype, step))
    assert pair.both(lambda c: c.sync()) == dict(zip(pair.ids, [75, 100, 87]))
    assert pair.both(lambda c: [len(c.pages[q]) for q in pair.ids]) == [3, 4, 3]      # two boundaries crossed each
    assert list(pair.caches[0].graphs) == [(3, False)]


@pytest.mark.parametrize("fused", [False, True])
def test_active_mask_freezes_a_sequence_then_sync(fused):
    model = _model("alt3")
    g = torch.Generator().manual_seed(5)
    ragged, paged = _Ragged(model, _prompts(6, LENS), fused), _Paged(model, _prompts(6, LENS), fused)
    on = torch.tensor([True, True, True], device=DEV)
    off = torch.tensor([True, False, True], device=DEV)
    for step, mask in enumerate([on] * 3 + [off] * 4):
        tok = _toks(g, 3)
        ragged.step(tok, mask, tag=("ragged", step))
        paged.step(paged.ids, tok, mask, tag=("paged", step))
    want = [5 + 7, 30 + 3, 17 + 7]
    for c in ragged.caches:
        assert c.host_exact is False and c.sync() == want
    assert paged.both(lambda c: c.sync()) == dict(zip(paged.ids, want))
    for step in range(3):                                   # and on without a mask: the other graph of this B
        tok = _toks(g, 3)
        ragged.step(tok, tag=("ragged after sync", step))
        paged.step(paged.ids, tok, tag=("paged after sync", step))
    assert sorted(ragged.caches[0].graphs) == sorted(paged.caches[0].graphs) == [(3, False), (3, True)]


@pytest.mark.parametrize("kv_dtype", [None, FP8])
def test_fork_then_a_step_that_copies_on_write(kv_dtype):
    model = _model("diff")
    pair = _Paged(model, _prompts(7, [40]), True, kv_dtype)            # a partial second page
    (root,) = pair.ids
    child = pair.both(lambda c: c.fork(root))
    g = torch.Generator().manual_seed(8)
    before = pair.both(lambda c: c.pages_in_use())
    for step in range(3):
        got = pair.step([root, child], _toks(g, 2), tag=("fork", kv_dtype, step))
    assert pair.both(lambda c: c.pages_in_use()) == before + 1           # the shared partial page was copied once
    assert pair.both(lambda c: c.pages[root][0] == c.pages[child][0] and c.pages[root][1] != c.pages[child][1])
    assert not torch.equal(got[0], got[1])                               # different tokens went in


def test_release_and_prefill_into_the_live_batch():
    model = _model("ctrl")
    pa, pb, pc = _prompts(9, [40, 20, 33])
    pair = _Paged(model, [pa, pb], True, pool=6)
    a, b = pair.ids
    g = torch.Generator().manual_seed(10)
    for step in range(3):
        pair.step([a, b], _toks(g, 2), tag=("A+B", step))
    pair.both(lambda c: c.release(a))
    (c,) = pair.prefill([pc])                                            # takes A's slot and pages
    for step in range(3):
        pair.step([b, c], _toks(g, 2), tag=("B+C", step))
    assert pair.both(lambda cc: cc.sync()) == {b: 26, c: 36}
    assert list(pair.caches[0].graphs) == [(2, False)]                   # one graph served both pairs


def test_another_order_and_a_smaller_subset():
    model = _model("alt3")
    pair = _Paged(model, _prompts(11, LENS), True)
    a, b, c = pair.ids
    g = torch.Generator().manual_seed(12)
    graphs = pair.caches[0].graphs
    for step in range(2):
        pair.step([a, b, c], _toks(g, 3), tag=("abc", step))
    for step in range(2):
        pair.step([c, a, b], _toks(g, 3), tag=("cab", step))             # the same B in another order: same graph
    assert list(graphs) == [(3, False)]
    for step in range(2):
        pair.step([b, c], _toks(g, 2), tag=("bc", step))                 # a second graph
    assert sorted(graphs) == [(2, False), (3, False)]
    first = graphs[(3, False)]
    for step in range(2):
        pair.step([b, a, c], _toks(g, 3), tag=("bac", step))             # and the first one is still right
    assert graphs[(3, False)] is first
    assert pair.both(lambda cc: cc.sync()) == {a: 5 + 6, b: 30 + 8, c: 17 + 8}


def test_truncate_then_continue():
    model = _model("diff")
    g = torch.Generator().manual_seed(13)
    ragged, paged = _Ragged(model, _prompts(14, LENS), True), _Paged(model, _prompts(14, LENS), True)
    a, b, c = paged.ids
    for step in range(4):
        tok = _toks(g, 3)
        ragged.step(tok, tag=("ragged", step))
        paged.step(paged.ids, tok, tag=("paged", step))
    held = ragged.caches[0].lengths
    for cache in ragged.caches:
        cache.truncate([9, 31, 2])
    assert ragged.caches[0].lengths is held                              # the graph's storage, updated in place
    paged.both(lambda cc: cc.truncate(b, 31))
    paged.both(lambda cc: cc.truncate(c, 2))
    for step in range(4):
        tok = _toks(g, 3)
        ragged.step(tok, tag=("ragged after truncate", step))
        paged.step(paged.ids, tok, tag=("paged after truncate", step))
    assert ragged.caches[0].lengths.tolist() == [13, 35, 6]
    assert paged.both(lambda cc: cc.sync()) == {a: 13, b: 35, c: 6}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_with_the_flags_returns_the_same_tokens(dtype):
    model = _model("alt3", dtype)
    prompts = _prompts(15, [12, 3, 31])

    def run(fn, **kw):
        torch.manual_seed(16)
        with torch.no_grad():
            return fn(model, prompts, 20, **kw)

    want = run(kv_cache.generate_paged, page_size=P)
    got = run(kv_cache.generate_paged, page_size=P, graph=True, fused_step=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and len(got) == len(want) == 3
    want = run(kv_cache.generate_ragged)
    for kw in (dict(graph=True), dict(graph=True, fused_step=True)):
        got = run(kv_cache.generate_ragged, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), kw
    eos = int(want[0][14])                                               # a token the first sequence does sample
    want = run(kv_cache.generate_ragged, eos_id=eos)                     # the active mask, on the device
    got = run(kv_cache.generate_ragged, eos_id=eos, graph=True, fused_step=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and len(want[0]) <= 15
    want = run(kv_cache.generate_paged, page_size=P, eos_id=eos, kv_dtype=FP8, n_samples=2)
    got = run(kv_cache.generate_paged, page_size=P, eos_id=eos, kv_dtype=FP8, n_samples=2, graph=True, fused_step=True)
    assert all(torch.equal(x, y) for xs, ys in zip(got, want) for x, y in zip(xs, ys))


def test_replay_is_real(monkeypatch):
    """After the capture, further steps at the same B never enter the Python model step."""
    model = _model("diff")
    calls = []
    inner = kv_cache._seq_model_step

    def counted(*args, **kwargs):
        calls.append(1)
        return inner(*args, **kwargs)

    ragged = kv_cache.RaggedKVCache(graph=True, fused_step=True)
    paged = kv_cache.PagedKVCache(POOL, P, graph=True, fused_step=True)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        kv_cache.prefill_ragged(model, _prompts(18, LENS), ragged)
        ids, _ = kv_cache.prefill_paged(model, _prompts(18, LENS), paged)
        monkeypatch.setattr(kv_cache, "_seq_model_step", counted)        # _ragged_model_step calls through this name
        monkeypatch.setattr(kv_cache, "_paged_model_step", counted)
        kv_cache.decode_ragged(model, _toks(g, 3), ragged)
        kv_cache.decode_paged(model, ids, _toks(g, 3), paged)
        assert len(calls) == 4                                           # warm-up and capture, once per cache
        for _ in range(5):
            kv_cache.decode_ragged(model, _toks(g, 3), ragged)
            kv_cache.decode_paged(model, ids[::-1], _toks(g, 3), paged)
        assert len(calls) == 4
    assert ragged.lengths.tolist() == [n + 6 for n in LENS] and paged.sync() == dict(zip(ids, [n + 6 for n in LENS]))


def test_a_graph_cache_needs_a_prefill_and_refuses_the_shared_plan():
    model = _model("diff")
    with pytest.raises(ValueError):
        kv_cache.decode_ragged(model, torch.zeros(2, 1, dtype=torch.long, device=DEV), kv_cache.RaggedKVCache(graph=True))
    with pytest.raises(ValueError, match="shared_decode"):
        kv_cache.generate_paged(model, _prompts(19, [4]), 2, graph=True, shared_decode=True)
