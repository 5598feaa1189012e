"""Time one token of ``decode_paged`` -- host work included -- with and without the graph-replayed
step (``graph=True``) and the fused row write (``fused_step=True``).

Method of tools/fp8_bench.py: one process, HIP events around ``inner`` back-to-back steps,
``repeats`` windows after ``warmup`` rounds, the arms taking turns inside every repeat, median
[min, max] per step.  The events bracket everything a step enqueues, so a step the host cannot
feed fast enough is timed at the host's pace: that is the point of the measurement.
Models (cfg1-sized, as tools/generate_bench.py, bf16, seeded, block_size 4352): a DiffTransformer
(12000, 384, 6 heads, 6 layers) and an AlternatingDiffTransformer of the same width with n_terms 3.
B in 1, 8, 64; the sequences' lengths spread evenly over 512 .. 4096 (B = 1: 2304, their mean);
page size 64; a bf16 pool and an fp8 (e4m3) pool.  Every arm has a cache of its own, prefilled with
the same prompts, and is fed the same token every step (the lengths grow by one per step).
  plain        flags off: the parent's code path, the baseline
  plain_again  the same arm a second time: |plain - plain_again| is the noise band
  fused        fused_step=True
  graph        graph=True
  both         graph=True, fused_step=True
Before the timing, one step of every arm is compared with ``plain``'s bit for bit.
``clears_band``: the arm's median lies below min(plain, plain_again) by more than the band.
Usage: python tools/step_graph_bench.py [--out profiles/step_graph_bench.json] [--repeats 10]
       [--warmup 2] [--inner 10] [--batches 1,8,64]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops, kv_cache  # noqa: E402
from differential_transformer_replication_amd import diff_transformer as D  # noqa: E402
from differential_transformer_replication_amd import Ndiff_transformer as ND  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
VOCAB, P, BLOCK = 12000, 64, 4096 + 256
ARMS = {"plain": {}, "fused": {"fused_step": True}, "graph": {"graph": True},
        "both": {"graph": True, "fused_step": True}, "plain_again": {}}
MODELS = {
    "DiffTransformer cfg1": lambda: D.DiffTransformer(VOCAB, 384, 6, 6, BLOCK, 0.0),
    "AlternatingDiffTransformer N=3": lambda: ND.AlternatingDiffTransformer(VOCAB, 384, 6, 6, BLOCK, 0.0, n_terms=3),
}


def _lengths(B):
    return [2304] if B == 1 else [512 + (4096 - 512) * b // (B - 1) for b in range(B)]


def _cache(model, prompts, steps, kv_dtype, flags):
    """A cache that holds the prompts and has the pages for ``steps`` more tokens; prefilled 8 prompts at a time."""
    need = sum(-(-(p.shape[0] + steps) // P) for p in prompts)
    cache = kv_cache.PagedKVCache(need, P, max_seqs=len(prompts), kv_dtype=kv_dtype, **flags)
    ids = []
    for s in range(0, len(prompts), 8):
        more, _ = kv_cache.prefill_paged(model, prompts[s:s + 8], cache)
        ids += more
    return cache, ids


@torch.no_grad()
def case(name, model, B, kv_dtype, repeats, warmup, inner):
    host = _lengths(B)
    g = torch.Generator().manual_seed(B)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n in host]
    tok = torch.randint(0, VOCAB, (B, 1), generator=g).to(DEV)
    steps = 1 + (warmup + repeats) * inner
    if max(host) + steps > BLOCK:
        raise SystemExit(f"{steps} steps from length {max(host)} cross block_size {BLOCK}")
    caches = {arm: _cache(model, prompts, steps, kv_dtype, flags) for arm, flags in ARMS.items()}
    first = {arm: kv_cache.decode_paged(model, ids, tok, c) for arm, (c, ids) in caches.items()}   # captures the graphs
    row = {"case": "decode_paged step", "model": name, "dtype": "bf16", "pool": kv_dtype or "bf16", "B": B,
           "lengths": host if B > 1 else host[0], "page_size": P, "block_size": BLOCK, "repeats": repeats,
           "warmup": warmup, "inner": inner,
           "logits_equal_plain": {arm: bool(torch.equal(first[arm], first["plain"])) for arm in ARMS if arm != "plain"}}
    fns = {arm: (lambda c=c, ids=ids: kv_cache.decode_paged(model, ids, tok, c)) for arm, (c, ids) in caches.items()}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    band = abs(row["plain_ms"] - row["plain_again_ms"])
    floor = min(row["plain_ms"], row["plain_again_ms"])
    row["band_ms"] = round(band, 5)
    for arm in ARMS:
        row[arm + "_tokens_per_s"] = round(B / row[arm + "_ms"] * 1e3, 1)
        if arm != "plain":
            row[arm + "_over_plain"] = round(row[arm + "_ms"] / row["plain_ms"], 4)
        if arm not in ("plain", "plain_again"):
            row[arm + "_clears_band"] = bool(row[arm + "_ms"] < floor - band)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_graph_bench needs the GPU: there is nothing to time without one")
    if not ops.kv_step_supported():
        raise SystemExit("the built library has no dta_kv_step_rows")
    rows = []
    for name, ctor in MODELS.items():
        torch.manual_seed(0)
        model = ctor().to(DEV).to(torch.bfloat16).eval()
        for B in (int(b) for b in args.batches.split(",")):
            for kv_dtype in (None, "fp8_e4m3"):
                rows.append(case(name, model, B, kv_dtype, args.repeats, args.warmup, args.inner))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
                if args.out:                      # after every case: a run cut short keeps what it measured
                    with open(args.out, "w") as fh:
                        json.dump(rows, fh, indent=1)
                        fh.write("\n")


if __name__ == "__main__":
    main()
