"""Time the sampling penalties: the torch composition a caller writes today against ``ops.penalize_rows``
(``dta_penalize_rows``), alone, followed by the sampler, and inside a ``decode_paged`` step -- bf16 logits of
V = 12000 columns, R in 1, 8, 64 sequences, token histories of 512 and 4096 tokens.

Method of tools/sample_bench.py: one process, HIP events around ``inner`` back-to-back calls, ``repeats``
windows after ``warmup`` rounds, the arms taking turns inside every repeat, median [min, max] per call, host
work included.
  torch              scatter_add counts over a (R, V) table, then the elementwise passes (repetition,
                     frequency / presence, bias, min-p floor)
  torch_again        the same arm a second time: |torch - torch_again| is the noise band
  kernel             ops.penalize_rows with the same parameters
  torch_sample       torch, then ops.sample_rows with top-k 50 / top-p 0.9
  kernel_sample      kernel, then the same ops.sample_rows
and per (B, history length) one ``decode_paged`` step of DiffTransformer cfg1 with ``graph=True,
fused_step=True`` followed by ``Sampler.sample``:
  step / step_again  as the generate loop runs it without penalties (their difference: the band)
  step_penalized     with ``ops.penalize_rows`` in front of the sampler and the history append after it
``kernel_clears_band``: the kernel arm lies below min(torch, torch_again) by more than the band.
Not measured here: V above the LDS table (the workspace path), fp16 / fp32 logits, a kernel trace.
Usage: python tools/penalty_bench.py [--out profiles/penalty_bench.json] [--repeats 20] [--warmup 3]
       [--inner 20] [--rows 1,8,64] [--hist 512,4096] [--no-steps]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops, kv_cache  # noqa: E402
from differential_transformer_replication_amd import diff_transformer as D  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
VOCAB, TOP_K, TOP_P, P, BLOCK = 12000, 50, 0.9, 64, 4096 + 256
THETA, PRES, FREQ, GAP = 1.3, 0.2, 0.4, -3.0


def torch_penalize(logits, hist, hlen, gen_start, bias):
    """The composition without the kernel: counts by scatter_add, then one elementwise pass per step."""
    R, V = logits.shape
    t = torch.arange(hist.shape[1], device=hist.device)[None, :]
    live = t < hlen[:, None]
    col = hist.long()
    seen = torch.zeros(R, V, dtype=torch.int32, device=hist.device).scatter_add_(1, col, live.int())
    cnt = torch.zeros(R, V, dtype=torch.int32, device=hist.device).scatter_add_(1, col, (live & (t >= gen_start[:, None])).int())
    x = logits.float()
    x = torch.where(seen > 0, torch.where(x > 0, x / THETA, x * THETA), x)
    x = torch.where(cnt > 0, x - FREQ * cnt.float() - PRES, x)
    x = x + bias
    m = x.max(dim=1, keepdim=True).values
    return torch.where(x >= m + GAP, x, torch.full_like(x, float("-inf")))


def _state(R, L, extra=0):
    g = torch.Generator().manual_seed(R + L)
    hist = torch.randint(0, VOCAB, (R, L + extra), generator=g).to(torch.int32).to(DEV)
    hlen = torch.full((R,), L, dtype=torch.int32, device=DEV)
    gen_start = torch.full((R,), L // 4, dtype=torch.int32, device=DEV)
    bias = torch.zeros(VOCAB, device=DEV)
    bias[:16] = float("-inf")
    return g, hist, hlen, gen_start, bias


@torch.no_grad()
def row_case(R, L, repeats, warmup, inner):
    g, hist, hlen, gen_start, bias = _state(R, L)
    logits = (torch.randn(R, VOCAB, generator=g) * 4).to(torch.bfloat16).to(DEV)
    offset = torch.zeros(R, dtype=torch.int64, device=DEV)
    by_torch = lambda: torch_penalize(logits, hist, hlen, gen_start, bias)                      # noqa: E731
    by_kernel = lambda: ops.penalize_rows(logits, hist, hlen, gen_start, None, None, THETA, PRES, FREQ, GAP, bias)   # noqa: E731
    sample = lambda x: ops.sample_rows(x, 1.0, TOP_K, TOP_P, seed=1, offset=offset)             # noqa: E731
    fns = {"torch": by_torch, "kernel": by_kernel, "torch_sample": lambda: sample(by_torch()),
           "kernel_sample": lambda: sample(by_kernel()), "torch_again": by_torch}
    row = {"case": "penalize rows", "dtype": "bf16", "R": R, "V": VOCAB, "history": L, "repeats": repeats,
           "warmup": warmup, "inner": inner,
           "max_abs_diff_kernel_torch": float((by_kernel() - by_torch()).nan_to_num(0.0, 0.0, 0.0).abs().max())}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    band = abs(row["torch_ms"] - row["torch_again_ms"])
    row["band_ms"] = round(band, 5)
    row["kernel_over_torch"] = round(row["kernel_ms"] / row["torch_ms"], 4)
    row["kernel_sample_over_torch_sample"] = round(row["kernel_sample_ms"] / row["torch_sample_ms"], 4)
    row["kernel_clears_band"] = bool(row["kernel_ms"] < min(row["torch_ms"], row["torch_again_ms"]) - band)
    return row


def _cache(model, prompts, steps):
    need = sum(-(-(p.shape[0] + steps) // P) for p in prompts)
    cache = kv_cache.PagedKVCache(need, P, max_seqs=len(prompts), graph=True, fused_step=True)
    ids = []
    for s in range(0, len(prompts), 8):
        more, _ = kv_cache.prefill_paged(model, prompts[s:s + 8], cache)
        ids += more
    return cache, ids


@torch.no_grad()
def step_case(model, B, L, repeats, warmup, inner):
    steps = 2 + (warmup + repeats) * inner
    if L + steps > BLOCK:
        raise SystemExit(f"{steps} steps from length {L} cross block_size {BLOCK}")
    g, hist, hlen, gen_start, bias = _state(B, L, extra=steps)
    prompts = [hist[b, :L].long() for b in range(B)]
    tok = torch.randint(0, VOCAB, (B, 1), generator=g).to(DEV)
    smp = kv_cache.Sampler(1.0, TOP_K, TOP_P, seed=1)
    caches = {arm: _cache(model, prompts, steps) for arm in ("step", "step_penalized", "step_again")}
    count = [0]

    def plain(arm):
        cache, ids = caches[arm]
        return smp.sample(kv_cache.decode_paged(model, ids, tok, cache), count[0])

    def penalized():
        cache, ids = caches["step_penalized"]
        logits = kv_cache.decode_paged(model, ids, tok, cache)
        out = smp.sample(ops.penalize_rows(logits, hist, hlen, gen_start, None, None, THETA, PRES, FREQ, GAP, bias), count[0])
        hist.scatter_(1, hlen.long()[:, None], out.to(torch.int32))
        hlen.add_(1)
        return out

    fns = {"step": lambda: plain("step"), "step_penalized": penalized, "step_again": lambda: plain("step_again")}
    for fn in fns.values():                                  # captures the graphs
        fn()
    row = {"case": "decode_paged step + sampler", "model": "DiffTransformer cfg1", "dtype": "bf16", "B": B, "V": VOCAB,
           "history": L, "page_size": P, "graph": True, "fused_step": True, "repeats": repeats, "warmup": warmup,
           "inner": inner}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    band = abs(row["step_ms"] - row["step_again_ms"])
    row["band_ms"] = round(band, 5)
    row["penalized_minus_step_ms"] = round(row["step_penalized_ms"] - row["step_ms"], 5)
    row["penalized_over_step"] = round(row["step_penalized_ms"] / row["step_ms"], 4)
    row["penalized_within_band"] = bool(row["step_penalized_ms"] <= max(row["step_ms"], row["step_again_ms"]) + band)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=10)
    ap.add_argument("--step-inner", type=int, default=10)
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--hist", default="512,4096")
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("penalty_bench needs the GPU: there is nothing to time without one")
    if not ops.penalize_rows_supported():
        raise SystemExit("the built library has no dta_penalize_rows")
    rows = []

    def keep(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.out:                                          # after every case: a run cut short keeps what it measured
            with open(args.out, "w") as fh:
                json.dump(rows, fh, indent=1)
                fh.write("\n")

    Rs, Ls = [int(r) for r in args.rows.split(",")], [int(n) for n in args.hist.split(",")]
    for L in Ls:
        for R in Rs:
            keep(row_case(R, L, args.repeats, args.warmup, args.inner))
    if not args.no_steps:
        torch.manual_seed(0)
        model = D.DiffTransformer(VOCAB, 384, 6, 6, BLOCK, 0.0).to(DEV).to(torch.bfloat16).eval()
        for L in Ls:
            for B in Rs:
                keep(step_case(model, B, L, args.step_repeats, 2, args.step_inner))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
