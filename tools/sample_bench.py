"""Time the last thing a token passes through: the reference's softmax + multinomial against
``ops.sample_rows`` (``dta_sample_rows``), on bf16 logits of V = 12000 columns, R in 1, 8, 64, 512.

Method of tools/step_graph_bench.py: one process, HIP events around ``inner`` back-to-back calls,
``repeats`` windows after ``warmup`` rounds, the arms taking turns inside every repeat, median
[min, max] per call, host work included.
  multinomial        F.softmax + torch.multinomial over the whole batch: the parent's lines
  multinomial_again  the same arm a second time: |multinomial - multinomial_again| is the noise band
  sorted_filter      a sort-based torch top-k 50 / top-p 0.9 filter, then softmax + multinomial
  sample             ops.sample_rows, unfiltered, with device offsets as the generate loops pass them
  sample_filtered    ops.sample_rows with top-k 50 / top-p 0.9
``sample_within_band``: the unfiltered kernel arm does not lie above max(multinomial, multinomial_again)
by more than the band.
Usage: python tools/sample_bench.py [--out profiles/sample_bench.json] [--repeats 20] [--warmup 3]
       [--inner 20] [--rows 1,8,64,512]
-> one JSON line per R (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
VOCAB, TOP_K, TOP_P = 12000, 50, 0.9


def sorted_filter(logits):
    """The filter callers write around ``decode_paged`` today: top-k by the k-th value, then the
    ascending cumulative probability <= 1 - p removed, then the reference's draw."""
    z = logits.float()
    z = z.masked_fill(z < z.topk(TOP_K, dim=-1).values[:, -1:], float("-inf"))
    zs, order = torch.sort(z, dim=-1)
    drop = F.softmax(zs, dim=-1).cumsum(-1) <= 1 - TOP_P
    drop[:, -1] = False
    z = z.masked_fill(torch.zeros_like(drop).scatter(1, order, drop), float("-inf"))
    return torch.multinomial(F.softmax(z, dim=-1), num_samples=1)


@torch.no_grad()
def case(R, repeats, warmup, inner):
    g = torch.Generator().manual_seed(R)
    logits = (torch.randn(R, VOCAB, generator=g) * 4).to(torch.bfloat16).to(DEV)
    offset = torch.zeros(R, dtype=torch.int64, device=DEV)
    plain = lambda: torch.multinomial(F.softmax(logits, dim=-1), num_samples=1)      # noqa: E731
    fns = {"multinomial": plain,
           "sorted_filter": lambda: sorted_filter(logits),
           "sample": lambda: ops.sample_rows(logits, seed=1, offset=offset),
           "sample_filtered": lambda: ops.sample_rows(logits, 1.0, TOP_K, TOP_P, seed=1, offset=offset),
           "multinomial_again": plain}
    row = {"case": "sample one token per row", "dtype": "bf16", "R": R, "V": VOCAB, "top_k": TOP_K, "top_p": TOP_P,
           "repeats": repeats, "warmup": warmup, "inner": inner}
    _report(row, interleaved_ms(fns, repeats, warmup, inner))
    band = abs(row["multinomial_ms"] - row["multinomial_again_ms"])
    row["band_ms"] = round(band, 5)
    row["sample_over_multinomial"] = round(row["sample_ms"] / row["multinomial_ms"], 4)
    row["sample_filtered_over_sorted_filter"] = round(row["sample_filtered_ms"] / row["sorted_filter_ms"], 4)
    row["sample_within_band"] = bool(row["sample_ms"] <= max(row["multinomial_ms"], row["multinomial_again_ms"]) + band)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rows", default="1,8,64,512")
    args = ap.parse_args()
    if not ops.sample_supported():
        raise SystemExit("the built library has no dta_sample_rows")
    rows = []
    for R in (int(r) for r in args.rows.split(",")):
        rows.append(case(R, args.repeats, args.warmup, args.inner))
        print(json.dumps(rows[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
