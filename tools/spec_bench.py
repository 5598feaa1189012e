"""Time speculative decoding on the paged cache -- host work included -- against the one-token step.

Method of tools/step_graph_bench.py: one process, HIP events around ``inner`` back-to-back calls, ``repeats``
windows after ``warmup`` rounds, the arms taking turns inside every repeat, median [min, max] per call.
Model: the cfg1-sized bf16 DiffTransformer (12000, 384, 6 heads, 6 layers, block_size 4352), seeded and
untrained -- so what prompt lookup would accept on it is about nothing and is not measured; the acceptance
rates below are forced.  B in 1, 8, 64; every sequence at length 512 or 4096; page size 64.
  (a) round    one round of K = 3 and K = 7 drafts (``append_paged(all_rows=True)`` of K + 1 rows on a
               ``rows_decode`` pool, ``ops.sample_rows`` of every row, ``ops.spec_accept_draft``, the read of
               the result, ``truncate`` to the old length + 1) against one eager ``decode_paged`` step, run
               twice (|eager - eager_again| is the noise band), and against the ``graph=True,
               fused_step=True`` step.  ``break_even_*``: round time / step time, the tokens a round has to
               emit per sequence to tie.
  (b) accept   the ``dta_spec_accept_draft`` launch against the same round state through a torch composition
               of it (batched tensor ops, no EOS handling), after checking that both give the same result.
  (c) generate ``generate_paged`` of ``--new`` tokens, greedy, plain against ``speculate`` with K = 3 and an
               oracle drafter that replays the recorded plain run: every draft right (rate 1), a miss at
               index 0 in every round (rate 0), or in every other round (rate 0.5).  Tokens per second of
               the whole call and with the time of a one-token call (the prefill) taken off; the rate
               reached (accepted / drafted) is reported next to the one asked for, since a bf16 round's
               logits need not pick the recorded token.
  (d) round_graph  section (a) again with the graph-replayed round (``Speculation(graph=True)``'s ``SpecRound`` on
               a ``rows_decode``, ``fused_step`` pool: pages and flush on the host, one replay, the read of the
               result, the host half of the roll-back) at K = 3 and K = 7 next to the eager round, the eager
               step twice and the ``graph=True, fused_step=True`` step, all taking turns inside every window.
               ``capture_ms_k*``: the warm-up and the capture, once per call, not part of a round's time.
               Not part of the default cases; its rows go to ``--graph-out``.
Usage: python tools/spec_bench.py [--out profiles/spec_bench.json] [--repeats 6] [--warmup 2] [--inner 5]
       [--batches 1,8,64] [--lengths 512,4096] [--new 48] [--cases accept,round,generate]
       python tools/spec_bench.py --cases round_graph --repeats 7 --inner 20
       [--graph-out profiles/spec_round_graph_bench.json]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops, kv_cache  # noqa: E402
from differential_transformer_replication_amd import diff_transformer as D  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
VOCAB, P, BLOCK = 12000, 64, 4096 + 256
SMP = kv_cache.Sampler(temperature=0)


def _cache(model, prompts, steps, **flags):
    need = sum(-(-(p.shape[0] + steps) // P) for p in prompts)
    cache = kv_cache.PagedKVCache(need, P, max_seqs=len(prompts), **flags)
    ids = []
    for s in range(0, len(prompts), 8):
        more, _ = kv_cache.prefill_paged(model, prompts[s:s + 8], cache)
        ids += more
    return cache, ids


def _round_fn(model, cache, ids, K, g):
    """One round with every draft slot filled; whatever is accepted, the cache keeps one row, so the
    lengths grow as the one-token arms' do."""
    B = len(ids)
    new_idx = torch.randint(0, VOCAB, (B, K + 1), generator=g).to(DEV)
    hist = torch.randint(0, VOCAB, (B, BLOCK), generator=g).to(DEV, torch.int32)
    hlen = torch.tensor([cache.host_lengths[q] + 1 for q in ids], dtype=torch.int32, device=DEV)
    draft = new_idx[:, 1:].to(torch.int32).contiguous()
    back = torch.zeros(3 * B, dtype=torch.int32, device=DEV)
    result, remaining = back[:2 * B].view(B, 2), back[2 * B:]
    dcnt = torch.full((B,), K, dtype=torch.int32, device=DEV)
    strm = torch.arange(B, device=DEV)[:, None].expand(B, K + 1).reshape(-1)
    off = torch.arange(K + 1, device=DEV)[None, :].expand(B, K + 1).reshape(-1)

    def fn():
        have = [cache.host_lengths[q] for q in ids]
        rows = kv_cache.append_paged(model, ids, new_idx, [K + 1] * B, cache, all_rows=True)
        tok = ops.sample_rows(rows, 0.0, 0, 1.0, 0, strm, off)
        remaining.fill_(1 << 20)
        dcnt.fill_(K)
        hlen.fill_(have[0] + 1)
        ops.spec_accept_draft(hist, hlen, remaining, draft, dcnt, tok, -1, K, 1, 3, BLOCK, result)
        back.tolist()
        for q, n in zip(ids, have):
            cache.truncate(q, n + 1)
    return fn


@torch.no_grad()
def round_case(model, B, length, repeats, warmup, inner):
    g = torch.Generator().manual_seed(B + length)
    prompts = [torch.randint(0, VOCAB, (length,), generator=g).to(DEV) for _ in range(B)]
    tok = torch.randint(0, VOCAB, (B, 1), generator=g).to(DEV)
    steps = 8 + 1 + (warmup + repeats) * inner
    arms = {"eager": {}, "round_k3": {"rows_decode": True}, "round_k7": {"rows_decode": True},
            "graph_fused": {"graph": True, "fused_step": True}, "eager_again": {}}
    caches = {arm: _cache(model, prompts, steps, **flags) for arm, flags in arms.items()}
    fns = {}
    for arm, (c, ids) in caches.items():
        if arm.startswith("round"):
            fns[arm] = _round_fn(model, c, ids, int(arm[-1]), g)
        else:
            fns[arm] = lambda c=c, ids=ids: kv_cache.decode_paged(model, ids, tok, c)
    for fn in fns.values():
        fn()                                       # captures the graph
    row = {"case": "round", "model": "DiffTransformer cfg1", "dtype": "bf16", "B": B, "length": length,
           "page_size": P, "repeats": repeats, "warmup": warmup, "inner": inner}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    row["band_ms"] = round(abs(row["eager_ms"] - row["eager_again_ms"]), 5)
    for k in (3, 7):
        r = row[f"round_k{k}_ms"]
        row[f"break_even_tokens_k{k}_vs_eager"] = round(r / row["eager_ms"], 3)
        row[f"break_even_tokens_k{k}_vs_graph_fused"] = round(r / row["graph_fused_ms"], 3)
    return row


def _graph_round_fn(model, cache, ids, K, g):
    """``_round_fn``'s round as ``Speculation(graph=True)`` runs it: the host takes the pages of the K + 1 rows
    and flushes, one ``SpecRound`` replay, the read of the result, the host half of the roll-back.  The draft is
    reset to random tokens before every round (one more small launch than the eager arm makes), so that the
    round's own lookup does not feed an untrained model its own repetitions and the cache grows by about one
    row a round, as the other arms' do.  Returns (fn, ms the warm-up and the capture took)."""
    B = len(ids)
    hist = torch.randint(0, VOCAB, (B, BLOCK), generator=g).to(DEV, torch.int32)
    hlen = torch.tensor([cache.host_lengths[q] + 1 for q in ids], dtype=torch.int32, device=DEV)
    draft0 = torch.randint(0, VOCAB, (B, K), generator=g).to(DEV, torch.int32)
    draft = draft0.clone()
    back = torch.zeros(3 * B, dtype=torch.int32, device=DEV)
    result, remaining = back[:2 * B].view(B, 2), back[2 * B:]
    dcnt = torch.full((B,), K, dtype=torch.int32, device=DEV)
    slots = torch.tensor([cache.slot[q] for q in ids], device=DEV)
    cache._flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rnd = kv_cache.SpecRound(model, cache, SMP, kv_cache.Speculation(k=K, graph=True),
                             (hist, hlen, remaining, draft, dcnt, result), 1 << 20, VOCAB, -1,
                             torch.arange(B, dtype=torch.int64, device=DEV), slots)
    torch.cuda.synchronize()
    capture_ms = (time.perf_counter() - t0) * 1e3

    def fn():
        have = [cache.host_lengths[q] for q in ids]
        remaining.fill_(1 << 20)
        dcnt.fill_(K)
        draft.copy_(draft0)
        hlen.fill_(min(have) + 1)
        cache._prepare_writes(ids, [n + K + 1 for n in have])
        cache._flush()
        rnd.run()
        m = back.tolist()[0:2 * B:2]
        for q, n, k in zip(ids, have, m):
            cache._rolled_back(q, n + k)
    return fn, capture_ms


@torch.no_grad()
def round_graph_case(model, B, length, repeats, warmup, inner):
    """Section (a)'s arms and the graph-replayed round next to them, taking turns inside every window."""
    g = torch.Generator().manual_seed(B + length)
    prompts = [torch.randint(0, VOCAB, (length,), generator=g).to(DEV) for _ in range(B)]
    tok = torch.randint(0, VOCAB, (B, 1), generator=g).to(DEV)
    steps = 16 + 1 + (warmup + repeats) * inner
    if length + steps + 8 > BLOCK:
        raise SystemExit(f"(warmup + repeats) * inner = {(warmup + repeats) * inner} rows do not fit the window")
    fast = {"rows_decode": True, "fused_step": True}
    arms = {"eager": {}, "round_k3": {"rows_decode": True}, "graph_round_k3": fast,
            "round_k7": {"rows_decode": True}, "graph_round_k7": fast,
            "graph_fused": {"graph": True, "fused_step": True}, "eager_again": {}}
    caches = {arm: _cache(model, prompts, steps, **flags) for arm, flags in arms.items()}
    fns, capture = {}, {}
    for arm, (c, ids) in caches.items():
        if arm.startswith("graph_round"):
            fns[arm], capture[arm] = _graph_round_fn(model, c, ids, int(arm[-1]), g)
        elif arm.startswith("round"):
            fns[arm] = _round_fn(model, c, ids, int(arm[-1]), g)
        else:
            fns[arm] = lambda c=c, ids=ids: kv_cache.decode_paged(model, ids, tok, c)
    for fn in fns.values():
        fn()                                       # captures the one-token graph
    row = {"case": "round_graph", "model": "DiffTransformer cfg1", "dtype": "bf16", "B": B, "length": length,
           "page_size": P, "repeats": repeats, "warmup": warmup, "inner": inner}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    row["band_ms"] = round(abs(row["eager_ms"] - row["eager_again_ms"]), 5)
    row["rows_grown"] = {arm: max(c.host_lengths.values()) - length for arm, (c, _) in caches.items()}
    for k in (3, 7):
        r, gr = row[f"round_k{k}_ms"], row[f"graph_round_k{k}_ms"]
        row[f"capture_ms_k{k}"] = round(capture[f"graph_round_k{k}"], 2)
        row[f"graph_round_k{k}_below_eager_round_ms"] = round(r - gr, 5)
        row[f"graph_round_k{k}_wins_by_more_than_band"] = bool(r - gr > row["band_ms"])
        row[f"break_even_tokens_k{k}_eager_round_vs_graph_fused"] = round(r / row["graph_fused_ms"], 3)
        row[f"break_even_tokens_k{k}_graph_round_vs_graph_fused"] = round(gr / row["graph_fused_ms"], 3)
    return row


def torch_composition(hist, hlen, remaining, draft, dcnt, tok, K, nmax, t_cap):
    """The kernel's round (ngram_min 1, no EOS) as batched torch ops, in place; returns (m, dcnt)."""
    B, cap = hist.shape
    j = torch.arange(K + 1, device=hist.device)
    agree = (tok[:, :K] == draft) & (j[None, :K] < dcnt[:, None])
    live = remaining > 0
    m = torch.minimum(agree.long().cumprod(1).sum(1) + 1, remaining.long()) * live
    at = (hlen[:, None].long() + j[None, :]).clamp_(max=cap - 1)
    hist.scatter_(1, at, torch.where(j[None, :] < m[:, None], tok.to(torch.int32), hist.gather(1, at)))
    L = hlen.long() + m
    rem = remaining.long() - m
    e = torch.arange(cap, device=hist.device)
    same = torch.ones(B, cap, dtype=torch.bool, device=hist.device)
    mu = torch.zeros(B, cap, dtype=torch.long, device=hist.device)
    for t in range(nmax):
        suf = hist.gather(1, (L - 1 - t).clamp_(min=0)[:, None])
        same = same & (torch.roll(hist, t, 1) == suf) & (e[None, :] >= t) & (L[:, None] - 1 - t >= 0)
        mu = mu + same
    key = torch.where((e[None, :] < L[:, None] - 1) & (mu >= 1), (mu << 32) | e[None, :], 0)
    best = key.max(1).values
    end = best & 0xFFFFFFFF
    nd = torch.minimum(torch.minimum(L - 1 - end, rem - 1), t_cap - L).clamp_(0, K) * (best > 0) * live * (rem > 1)
    src = (end[:, None] + 1 + j[None, :K]).clamp_(max=cap - 1)
    draft.copy_(torch.where(j[None, :K] < nd[:, None], hist.gather(1, src), draft))
    hlen.copy_(torch.where(live, L, hlen.long()))
    remaining.copy_(torch.where(live, rem, remaining.long()))
    dcnt.copy_(torch.where(live, nd, dcnt.long()))
    return torch.stack([m, nd], dim=1).to(torch.int32)


def accept_case(B, length, K, repeats, warmup, inner):
    g = torch.Generator().manual_seed(7 * B + length + K)
    cap = BLOCK
    base = dict(hist=torch.randint(0, 50, (B, cap), generator=g).to(DEV, torch.int32),
                hlen=torch.full((B,), length, dtype=torch.int32, device=DEV),
                remaining=torch.full((B,), 1000, dtype=torch.int32, device=DEV),
                draft=torch.randint(0, 50, (B, K), generator=g).to(DEV, torch.int32),
                dcnt=torch.full((B,), K, dtype=torch.int32, device=DEV))
    tok = torch.randint(0, 50, (B, K + 1), generator=g).to(DEV)
    tok[::2, :K] = base["draft"][::2].long()
    one, two = {k: v.clone() for k, v in base.items()}, {k: v.clone() for k, v in base.items()}
    res = ops.spec_accept_draft(*one.values(), tok, -1, K, 1, 3, BLOCK)
    res2 = torch_composition(*two.values(), tok, K, 3, BLOCK)
    live = torch.arange(K, device=DEV)[None, :] < one["dcnt"][:, None]
    same = bool(torch.equal(res, res2)) and all(torch.equal(one[k], two[k]) for k in ("hist", "hlen", "remaining", "dcnt")) \
        and bool(torch.equal(torch.where(live, one["draft"], 0), torch.where(live, two["draft"], 0)))
    result = torch.empty(B, 2, dtype=torch.int32, device=DEV)

    def reset(s):
        s["hlen"].fill_(length)
        s["remaining"].fill_(1000)
        s["dcnt"].fill_(K)

    def kernel():
        reset(one)
        ops.spec_accept_draft(*one.values(), tok, -1, K, 1, 3, BLOCK, result)

    def composition():
        reset(two)
        torch_composition(*two.values(), tok, K, 3, BLOCK)

    row = {"case": "accept", "B": B, "length": length, "K": K, "ngram": [1, 3], "composition_equals_kernel": same,
           "repeats": repeats, "warmup": warmup, "inner": inner}
    _report(row, interleaved_ms({"kernel": kernel, "composition": composition, "kernel_again": kernel}, repeats, warmup, inner))
    row["composition_over_kernel"] = round(row["composition_ms"] / row["kernel_ms"], 2)
    return row


class ReplayDrafter:
    """Proposes the recorded run's next tokens, on the device; ``miss_every`` n > 0: in every n-th round the
    first draft is wrong (0: never)."""

    def __init__(self, plain, miss_every):
        self.plain = torch.nn.utils.rnn.pad_sequence(plain, batch_first=True).to(DEV, torch.int32)
        self.ends = torch.tensor([len(p) for p in plain], device=DEV)
        self.miss_every, self.round = miss_every, 0

    def propose(self, hist, hlen, remaining, k):
        at = hlen[:, None].long() + torch.arange(k, device=DEV)[None, :]
        draft = self.plain.gather(1, at.clamp(max=self.plain.shape[1] - 1))
        self.round += 1
        if self.miss_every and self.round % self.miss_every == 0:
            draft[:, 0] = (draft[:, 0] + 1) % VOCAB
        return draft, (self.ends - hlen).clamp(0, k).to(torch.int32)


@torch.no_grad()
def generate_case(model, B, length, new, repeats):
    g = torch.Generator().manual_seed(3 * B + length)
    prompts = [torch.randint(0, VOCAB, (length,), generator=g).to(DEV) for _ in range(B)]

    def timed(n, **kw):
        best, out = None, None
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = kv_cache.generate_paged(model, prompts, n, sampler=SMP, page_size=P, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, out

    timed(2)                                          # warm-up
    t_prefill, _ = timed(1)
    t_plain, plain = timed(new)
    t_graph, _ = timed(new, graph=True, fused_step=True)
    row = {"case": "generate", "model": "DiffTransformer cfg1", "dtype": "bf16", "B": B, "length": length, "new_tokens": new,
           "K": 3, "repeats_best_of": repeats, "prefill_s": round(t_prefill, 4),
           "plain_tokens_per_s": round(B * new / t_plain, 1),
           "plain_decode_tokens_per_s": round(B * (new - 1) / max(t_plain - t_prefill, 1e-9), 1),
           "graph_fused_decode_tokens_per_s": round(B * (new - 1) / max(t_graph - t_prefill, 1e-9), 1)}
    for rate, every in ((1.0, 0), (0.5, 2), (0.0, 1)):
        best, stats, equal = None, None, None
        for _ in range(repeats):
            spec = kv_cache.Speculation(k=3, drafter=ReplayDrafter(plain, every))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = kv_cache.generate_paged(model, prompts, new, sampler=SMP, page_size=P, speculate=spec)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if best is None or dt < best:
                best, stats = dt, dict(spec.stats)
            equal = all(torch.equal(a, b) for a, b in zip(out, plain))
        tag = f"rate_{rate}"
        row[tag + "_tokens_per_s"] = round(B * new / best, 1)
        row[tag + "_decode_tokens_per_s"] = round(B * (new - 1) / max(best - t_prefill, 1e-9), 1)
        row[tag + "_reached"] = round(stats["accepted"] / max(stats["drafted"], 1), 3)
        row[tag + "_rounds"] = stats["rounds"]
        row[tag + "_tokens_equal_plain"] = equal
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--lengths", default="512,4096")
    ap.add_argument("--new", type=int, default=48)
    ap.add_argument("--cases", default="accept,round,generate")
    ap.add_argument("--graph-out", default="profiles/spec_round_graph_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_bench needs the GPU: there is nothing to time without one")
    if not ops.spec_supported():
        raise SystemExit("the built library has no dta_spec_accept_draft")
    torch.manual_seed(0)
    model = D.DiffTransformer(VOCAB, 384, 6, 6, BLOCK, 0.0).to(DEV).to(torch.bfloat16).eval()
    rows, graph_rows = [], []

    def keep(row, rows=rows, out=args.out):
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        if out:                                       # after every case: a run cut short keeps what it measured
            with open(out, "w") as fh:
                json.dump(rows, fh, indent=1)
                fh.write("\n")

    batches = [int(b) for b in args.batches.split(",")]
    lengths = [int(n) for n in args.lengths.split(",")]
    cases = args.cases.split(",")
    shapes = [(B, length) for B in batches for length in lengths]
    if "accept" in cases:
        for B, length in shapes:
            for K in (3, 7):
                keep(accept_case(B, length, K, args.repeats, args.warmup, 4 * args.inner))
    if "round" in cases:
        for B, length in shapes:
            keep(round_case(model, B, length, args.repeats, args.warmup, args.inner))
    if "generate" in cases:
        for B, length in shapes:
            keep(generate_case(model, B, length, args.new, 2))
    if "round_graph" in cases:
        if not ops.spec_round_supported():
            raise SystemExit("the built library has no dta_spec_feed_rows / dta_spec_commit_lengths")
        for B, length in shapes:
            keep(round_graph_case(model, B, length, args.repeats, args.warmup, args.inner), graph_rows, args.graph_out)


if __name__ == "__main__":
    main()
