"""Helpers of the speculative-decoding tests: a brute-force Python reading of include/diffattn.h's
"Speculative decoding", random round states, a table-lookup model step for the ragged and the paged
loop (several rows per sequence, logits a function of a row's token and position alone, so they do not
depend on the step's shape), and an oracle drafter that proposes a recorded plain run's tokens with a
miss planted at a chosen index."""
import torch

from differential_transformer_replication_amd import kv_cache, ops

VOCAB = 13


# ------------------------------------------------------------------ the definition ---
def brute_force(hist, hlen, remaining, draft, dcnt, tok, eos_id, K, nmin, nmax, t_cap):
    """One row of one round on Python lists, written from the definition line by line (no clamps: valid
    state only).  Returns the new (hist, hlen, remaining, draft, dcnt, m)."""
    hist, draft = list(hist), list(draft)
    if remaining <= 0:
        return hist, hlen, remaining, draft, dcnt, 0
    Tn = len(tok)
    a = 0
    while a < min(dcnt, max(Tn - 1, 0)) and tok[a] == draft[a]:
        a += 1
    m = min(a + 1, remaining, Tn)
    stop = False
    for j in range(m):
        if tok[j] == eos_id or tok[j] < 0:
            m, stop = j + 1, True
            break
    remaining = 0 if stop else remaining - m
    hist[hlen:hlen + m] = tok[:m]
    hlen += m
    L = hlen
    if nmin == 0 or remaining <= 1 or L <= nmin:
        return hist, hlen, remaining, draft, 0, m
    best = None
    for e in range(nmin - 1, L - 1):
        mu = 0
        for n in range(1, min(nmax, e + 1) + 1):
            if all(hist[e - t] == hist[L - 1 - t] for t in range(n)):
                mu = n
            else:
                break
        if mu >= nmin and (best is None or (mu, e) > best):
            best = (mu, e)
    if best is None:
        return hist, hlen, remaining, draft, 0, m
    e = best[1]
    dcnt = max(min(K, L - 1 - e, remaining - 1, t_cap - L), 0)
    draft[:dcnt] = hist[e + 1:e + 1 + dcnt]
    return hist, hlen, remaining, draft, dcnt, m


def i32(x, device="cpu"):
    return torch.tensor(x, dtype=torch.int32, device=device)


class State:
    """The tensors of one ``ops.spec_accept_draft`` call."""

    def __init__(self, hist, hlen, remaining, draft, dcnt, tok):
        self.hist, self.hlen, self.remaining, self.draft, self.dcnt, self.tok = hist, hlen, remaining, draft, dcnt, tok

    def clone(self, device=None):
        return State(*(None if t is None else t.clone() if device is None else t.to(device).clone()
                       for t in self.tensors()))

    def tensors(self):
        return self.hist, self.hlen, self.remaining, self.draft, self.dcnt, self.tok

    def run(self, fn, eos_id, K, nmin, nmax, t_cap):
        return fn(self.hist, self.hlen, self.remaining, self.draft, self.dcnt, self.tok, eos_id, K, nmin, nmax, t_cap)


def random_state(B, hlens, cap, vocab, K, seed, eos_rate=0.0):
    """Valid state of B rows whose history lengths cycle through ``hlens``: drafts that mostly match
    their samples (so every acceptance count occurs), a few finished rows, remaining from 1 up."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape=(B,): torch.randint(lo, hi, shape, generator=g)      # noqa: E731
    hist = ri(0, vocab, (B, cap)).to(torch.int32)
    hlen = i32([hlens[b % len(hlens)] for b in range(B)])
    remaining = torch.minimum(ri(1, 12), cap - hlen.long()).to(torch.int32)
    remaining[ri(0, 8) == 0] = 0
    dcnt = ri(0, K + 1).to(torch.int32)
    draft = ri(0, vocab, (B, K)).to(torch.int32)
    tok = ri(0, vocab, (B, K + 1))
    agree = ri(0, K + 2)                                  # the leading drafts that equal their samples
    for b in range(B):
        n = int(agree[b])
        tok[b, :min(n, K)] = draft[b, :min(n, K)]
    if eos_rate:
        tok[torch.rand(B, K + 1, generator=g) < eos_rate] = -1
    return State(hist, hlen, remaining, draft, dcnt, tok)


def check_against_brute_force(st, eos_id, K, nmin, nmax, t_cap):
    """``ops.spec_accept_draft_reference`` on a copy of ``st`` against ``brute_force`` row by row; returns
    the acceptance counts m it saw."""
    got = st.clone()
    res = got.run(ops.spec_accept_draft_reference, eos_id, K, nmin, nmax, t_cap)
    seen = set()
    for b in range(st.hist.shape[0]):
        tok = [] if st.tok is None else st.tok[b].tolist()
        h, L, rem, d, dc, m = brute_force(st.hist[b].tolist(), int(st.hlen[b]), int(st.remaining[b]), st.draft[b].tolist(),
                                          int(st.dcnt[b]), tok, eos_id, K, nmin, nmax, t_cap)
        live = int(st.remaining[b]) > 0
        assert res[b].tolist() == [m, dc if live else 0], b
        assert got.hist[b].tolist() == h and int(got.hlen[b]) == L and int(got.remaining[b]) == rem, b
        assert got.draft[b].tolist() == d and int(got.dcnt[b]) == dc, b
        seen.add(m)
    return seen


# ------------------------------------------------------------------ the loops ---
class Model:
    block_size = 64


def prompts(*lens):
    return [(torch.arange(n, dtype=torch.long) * 7 + n) % VOCAB for n in lens]


def stub_steps(monkeypatch, device="cpu", seed=5):
    """Replace the ragged and the paged model step by a table lookup: row r of sequence b gives
    table[token] + 0.01 * position, whatever else is in the step."""
    table = (torch.randn(VOCAB, VOCAB, generator=torch.Generator().manual_seed(seed)) * 3).to(device)

    def step(idx, pos, gather):
        if gather is not None and pos is None:                  # a prefill: each sequence's last real row
            last = idx.gather(1, gather[:, None])[:, 0]
            return table[last] + 0.01 * gather[:, None]
        at = pos[:, None].long() + torch.arange(idx.shape[1], device=idx.device)[None, :]
        out = table[idx] + 0.01 * at[..., None]
        return out if gather is None else out[torch.arange(idx.shape[0], device=idx.device), gather]

    def ragged(model, idx, cache, pos, counts, gather=None, one_row=False):
        return step(idx, pos, gather)

    def paged(model, idx, cache, tbl, pos, counts, gather=None, one_row=False):
        return step(idx, pos, gather)

    monkeypatch.setattr(kv_cache, "_ragged_model_step", ragged)
    monkeypatch.setattr(kv_cache, "_paged_model_step", paged)
    return table


class OracleDrafter:
    """Proposes what the plain run emitted next (``plain``: its outputs, prompts included), with a wrong
    token at draft index ``miss(round, b)`` (None or >= k: none), so a round accepts exactly that many."""

    def __init__(self, plain, vocab, miss):
        self.plain, self.vocab, self.miss, self.round = plain, vocab, miss, 0

    def propose(self, hist, hlen, remaining, k):
        B = hist.shape[0]
        draft = torch.zeros(B, k, dtype=torch.int32)
        dcnt = torch.zeros(B, dtype=torch.int32)
        for b, L in enumerate(hlen.tolist()):
            nxt = self.plain[b][L:L + k].tolist()
            at = self.miss(self.round, b)
            if at is not None and at < len(nxt):
                nxt[at] = (nxt[at] + 1) % self.vocab
            draft[b, :len(nxt)] = torch.tensor(nxt, dtype=torch.int32)
            dcnt[b] = len(nxt)
        self.round += 1
        return draft.to(hist.device), dcnt.to(hist.device)


class RecordingPagedCache(kv_cache.PagedKVCache):
    """``generate_paged`` makes its own cache: this one remembers the last made."""
    last = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        RecordingPagedCache.last = self
