"""Helpers of the fixed-shape speculative round's tests: a line-by-line Python reading of include/diffattn.h's
"A fixed-shape speculative round" (``dta_spec_feed_rows``, ``dta_spec_commit_lengths``), the states both test
files run (``_spec.random_state`` plus edge rows: finished rows, an empty and a full history, no draft and a full
one, and device values out of range), and the inputs of the length commit."""
import torch

import _spec as S

CAP, VOCAB, TOTAL = 40, 13, 12
HLENS = [1, 2, 5, 9, 17, 30, 38]
BATCHES, KS = (1, 3, 64), (1, 3, 7)
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


# ------------------------------------------------------------------ the definition ---
def clamp(x, lo, hi):
    return min(max(x, lo), hi)


def definition_feed(hist, hlen, remaining, draft, dcnt, K, cap, vocab, total):
    """One row on Python integers: (idx_out[b] (K + 1), counts_out[b], offset_out[b] (K + 1))."""
    T = K + 1
    L = clamp(hlen, 0, cap)
    live = remaining > 0 and L >= 1
    d = clamp(dcnt, 0, K) if live else 0
    counts = d + 1 if live else 0
    idx = [0] * T
    idx[0] = clamp(hist[L - 1], 0, vocab - 1) if live else 0
    for j in range(1, K + 1):
        idx[j] = clamp(draft[j - 1], 0, vocab - 1) if j <= d else 0
    offset = [(total - remaining) + j for j in range(T)]
    return idx, counts, offset


def definition_commit(lengths, result, K, t_cap, slots):
    """The whole of ``lengths`` after the launch, on Python integers."""
    lengths = list(lengths)
    for b in range(len(result)):
        s = clamp(slots[b], 0, len(lengths) - 1) if slots is not None else b
        lengths[s] = min(lengths[s] + clamp(result[b][0], 0, K + 1), t_cap)
    return lengths


def check_feed(st, K, idx, counts, offset, total=TOTAL, vocab=VOCAB):
    """(idx, counts, offset) as tensors against ``definition_feed`` row by row."""
    cap = st.hist.shape[1]
    for b in range(st.hist.shape[0]):
        want = definition_feed(st.hist[b].tolist(), int(st.hlen[b]), int(st.remaining[b]), st.draft[b].tolist(),
                               int(st.dcnt[b]), K, cap, vocab, total)
        assert (idx[b].tolist(), int(counts[b]), offset[b].tolist()) == want, (b, want)


# ------------------------------------------------------------------ the states ---
def edge_rows(K, cap=CAP, vocab=VOCAB, total=TOTAL):
    """(hlen, remaining, dcnt, draft or None, pending token or None): each overrides one row of a state."""
    return [(9, 0, 2, None, None), (9, -3, K, None, None), (9, I32_MIN, 1, None, None),   # finished
            (0, 5, 1, None, None), (cap, 5, K, None, None),                               # no history, a full one
            (17, 5, 0, None, None), (17, 5, K, None, None),                               # no draft, a full one
            (-4, 5, 1, None, None), (cap + 1000, 5, 1, None, 3), (I32_MAX, 2, K, None, None),   # hlen out of range
            (9, 5, K + 50, None, None), (9, 5, -2, None, None), (9, 5, I32_MAX, None, None),    # dcnt out of range
            (9, 5, K, [-5] * K, None), (9, 5, K, [vocab + 7] * K, None), (9, 5, K, [I32_MIN, I32_MAX] * 4, None),
            (9, 5, 1, None, -9), (9, 5, 1, None, vocab), (30, 5, K, None, I32_MAX),       # tokens out of range
            (9, total + 5, 1, None, None), (9, I32_MAX, 1, None, None)]                   # more owed than the call's total


def states(B, K, seed=0):
    """The random valid state of B rows, then copies of it whose leading rows are the edge rows, B at a time."""
    st = S.random_state(B, HLENS, CAP, VOCAB, K, seed=1000 * K + B + seed)
    yield "valid", st
    edges = edge_rows(K)
    for at in range(0, len(edges), B):
        e = st.clone()
        for b, (hlen, rem, dcnt, draft, pending) in enumerate(edges[at:at + B]):
            e.hlen[b], e.remaining[b], e.dcnt[b] = hlen, rem, dcnt
            if draft is not None:
                e.draft[b] = S.i32(draft[:K])
            if pending is not None:
                e.hist[b, S_clamp(hlen) - 1] = pending
        yield f"edges {at}", e


def S_clamp(hlen):
    return clamp(hlen, 1, CAP)


def commit_inputs(B, K, t_cap, paged, seed=0):
    """(lengths, result, slots or None) on the CPU: m in and out of 0 .. K + 1, lengths at and next to ``t_cap``,
    and paged, distinct slots of a longer ``lengths`` with one below and one above its range."""
    g = torch.Generator().manual_seed(77 * K + B + seed)
    n_slots = B + 5 if paged else B
    lengths = torch.randint(0, t_cap - K - 1, (n_slots,), generator=g).to(torch.int32)
    lengths[::4] = t_cap
    lengths[1::5] = t_cap - 1
    result = torch.randint(0, K + 2, (B, 2), generator=g).to(torch.int32)
    wild = [-3, K + 2, I32_MAX, I32_MIN, K + 1, 0]
    for b in range(min(B, len(wild))):
        result[(b * 7) % B, 0] = wild[b]
    slots = None
    if paged:
        slots = (torch.randperm(n_slots - 2, generator=g)[:B] + 1).long()       # 1 .. n_slots - 2, distinct
        slots[0] = -7                                                            # clamps to slot 0
        if B > 1:
            slots[1] = n_slots + 9                                               # clamps to the last slot
    return lengths, result, slots
