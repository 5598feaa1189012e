"""Time the ragged-batch kernels over the KV cache (``ops.diff_attention_decode_ragged``,
``ops.diff_attention_extend_ragged``) against what a caller had to do without them.

Shape: the cfg2 head shape (H=16, hs=64, dv=128, N=2, bf16), B=8, t_cap=4096.  Arms, all
timed with HIP events in one process, interleaved round-robin (every repeat runs every
arm once, so drift hits all arms alike), median / min / max of the repeats after warm-up;
each timed window is ``inner`` back-to-back calls, reported per call:
  (1) ragged          one ragged decode, lengths spread evenly from 512 to 4096
  (2) uniform_padded  the one-length decode at 4096 for every sequence: what a padded
                      batch costs today (and it attends to the padding: wrong answers)
  (3) per_sequence    B separate B=1 decodes at each sequence's own length: the only
                      correct route today
  (4) ragged_full     the ragged decode with every length 4096 -- against arm (2), the
                      cost of reading the length per sequence; arm (2) runs twice per
                      repeat (uniform_padded, uniform_again) and the spread between its
                      two copies is the noise band
  (5) extend_ragged   one ragged extend, Tq=64, positions spread evenly from 448 to 4032,
                      against extend_per_sequence: B separate B=1 one-position extends
Usage: python tools/ragged_bench.py [--out FILE] [--repeats 50] [--warmup 10] [--inner 20]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops  # noqa: E402

DEV = "cuda"


def interleaved_ms(arms, repeats, warmup, inner):
    """arms: {name: fn}.  Per-call ms of every arm: (median, min, max) over ``repeats``
    windows of ``inner`` calls, the arms taking turns inside every repeat."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / inner)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def _report(row, stats):
    for name, (med, lo, hi) in stats.items():
        row[name + "_ms"] = round(med, 5)
        row[name + "_ms_min_max"] = [round(lo, 5), round(hi, 5)]


def decode_case(repeats, warmup, inner):
    B, H, N, hs, cap = 8, 16, 2, 64, 4096
    dv = 2 * hs
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(B, cap, ops.packed_width(H, N, hs, dv), device=DEV, generator=g).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    q, k, v = ops.split_packed(qkv, H, N, hs, dv)
    q1 = q[:, -1]
    host = [512 + (cap - 512) * b // (B - 1) for b in range(B)]
    lengths = torch.tensor(host, dtype=torch.int32, device=DEV)
    full = torch.full((B,), cap, dtype=torch.int32, device=DEV)
    one = [lengths[b:b + 1] for b in range(B)]

    # the arms compute the same thing where they should
    rag = ops.diff_attention_decode_ragged(q1, k, v, coef, lengths)
    per = torch.cat([ops.diff_attention_decode(q1[b:b + 1], k[b:b + 1], v[b:b + 1], coef, host[b]) for b in range(B)])
    uni = ops.diff_attention_decode(q1, k, v, coef, cap)
    row = {"case": "decode", "dtype": "bf16", "B": B, "H": H, "head_size": hs, "dv": dv, "n_terms": N, "t_cap": cap,
           "lengths": host, "traffic_fraction": round(sum(host) / (B * cap), 4), "repeats": repeats, "warmup": warmup,
           "inner": inner,
           "ragged_equals_per_sequence": bool(torch.equal(rag, per)),
           "ragged_full_equals_uniform": bool(torch.equal(ops.diff_attention_decode_ragged(q1, k, v, coef, full), uni))}

    def per_sequence():
        for b in range(B):
            ops.diff_attention_decode(q1[b:b + 1], k[b:b + 1], v[b:b + 1], coef, host[b])

    arms = {
        "ragged": lambda: ops.diff_attention_decode_ragged(q1, k, v, coef, lengths),
        "uniform_padded": lambda: ops.diff_attention_decode(q1, k, v, coef, cap),
        "per_sequence": per_sequence,
        "ragged_full": lambda: ops.diff_attention_decode_ragged(q1, k, v, coef, full),
        "uniform_again": lambda: ops.diff_attention_decode(q1, k, v, coef, cap),
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    row["ragged_over_uniform_padded"] = round(row["ragged_ms"] / row["uniform_padded_ms"], 4)
    row["per_sequence_over_ragged"] = round(row["per_sequence_ms"] / row["ragged_ms"], 3)
    row["ragged_full_over_uniform"] = round(row["ragged_full_ms"] / row["uniform_padded_ms"], 4)
    row["uniform_again_over_uniform"] = round(row["uniform_again_ms"] / row["uniform_padded_ms"], 4)
    return row


def extend_case(repeats, warmup, inner):
    B, H, N, hs, cap, Tq = 8, 16, 2, 64, 4096, 64
    dv = 2 * hs
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = torch.randn(B, cap, ops.packed_width(H, N, hs, dv), device=DEV, generator=g).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    q, k, v = ops.split_packed(qkv, H, N, hs, dv)
    qn = q[:, :Tq]
    host = [448 + (cap - Tq - 448) * b // (B - 1) for b in range(B)]
    pos = torch.tensor(host, dtype=torch.int32, device=DEV)

    rag = ops.diff_attention_extend_ragged(qn, k, v, coef, pos)
    per = torch.cat([ops.diff_attention_extend(qn[b:b + 1], k[b:b + 1], v[b:b + 1], coef, host[b]) for b in range(B)])
    row = {"case": "extend", "dtype": "bf16", "B": B, "H": H, "head_size": hs, "dv": dv, "n_terms": N, "t_cap": cap,
           "Tq": Tq, "pos": host, "repeats": repeats, "warmup": warmup, "inner": inner,
           "ragged_equals_per_sequence": bool(torch.equal(rag, per))}

    def per_sequence():
        for b in range(B):
            ops.diff_attention_extend(qn[b:b + 1], k[b:b + 1], v[b:b + 1], coef, host[b])

    arms = {
        "extend_ragged": lambda: ops.diff_attention_extend_ragged(qn, k, v, coef, pos),
        "extend_per_sequence": per_sequence,
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    row["per_sequence_over_ragged"] = round(row["extend_per_sequence_ms"] / row["extend_ragged_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench needs the GPU: there is nothing to time without one")
    rows = []
    for case in (decode_case, extend_case):
        rows.append(case(args.repeats, args.warmup, args.inner))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
