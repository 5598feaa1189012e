"""Time the multi-row step over the KV cache (``ops.diff_attention_extend``) against
the two routes to the same rows that exist without it, and measure what a chunked
prefill saves in memory.

Timing legs: bf16, B=8, H=16, hs=64, dv=128, N=2, cache at L=4096, Tq in {8, 64, 256,
1024} new rows appended at pos = L - Tq, each timed three ways with HIP events in one
process (median of the timed repeats after warm-up):
  (a) extend   one ``diff_attention_extend`` launch
  (b) full     ``ops.diff_attention`` under no_grad over all L rows (re-prefill)
  (c) decode   Tq successive ``diff_attention_decode`` calls
Memory leg: the cfg5 shape (B=1, H=16, hs=128, dv=256, N=2, T=32768, bf16), one
attention layer (projection, attention, cache write) prefilled in one shot and in
chunks of 2048: peak allocated bytes above the resident inputs, weight and cache.
Usage: python tools/extend_bench.py [--out FILE] [--repeats 20] [--warmup 5]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import statistics
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import kv_cache, ops  # noqa: E402

DEV = "cuda"


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def timing_legs(repeats, warmup):
    B, H, N, hs, L = 8, 16, 2, 64, 4096
    dv = 2 * hs
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(B, L, ops.packed_width(H, N, hs, dv), device=DEV, generator=g).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    q, k, v = ops.split_packed(qkv, H, N, hs, dv)
    with torch.no_grad():
        full = ops.diff_attention(qkv, coef, H, N, hs)
    for Tq in (8, 64, 256, 1024):
        pos = L - Tq
        ext = ops.diff_attention_extend(q[:, pos:], k, v, coef, pos)
        err = ((ext.float() - full[:, pos:].float()).abs().max() / full[:, pos:].float().abs().max()).item()

        def leg_a():
            ops.diff_attention_extend(q[:, pos:], k, v, coef, pos)

        def leg_b():
            with torch.no_grad():
                ops.diff_attention(qkv, coef, H, N, hs)

        def leg_c():
            for r in range(Tq):
                ops.diff_attention_decode(q[:, pos + r], k, v, coef, pos + r + 1)

        row = {"case": "timing", "dtype": "bf16", "B": B, "H": H, "head_size": hs, "dv": dv, "n_terms": N, "L": L,
               "Tq": Tq, "pos": pos, "repeats": repeats, "warmup": warmup, "extend_vs_full_rel_err": err}
        for name, fn in (("extend", leg_a), ("full_forward", leg_b), ("decode_loop", leg_c)):
            med, lo, hi = median_ms(fn, repeats, warmup)
            row[name + "_ms"] = round(med, 4)
            row[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        row["speedup_vs_full_forward"] = round(row["full_forward_ms"] / row["extend_ms"], 2)
        row["speedup_vs_decode_loop"] = round(row["decode_loop_ms"] / row["extend_ms"], 2)
        yield row


def _layer_prefill(x, weight, buf, coef, H, N, hs, dv, chunk):
    """One attention layer's cached prefill (kv_cache._attention_step without the model
    around it): rows [0, chunk) through the training forward, the rest appended."""
    T, nq = x.shape[1], H * N * hs
    for s in range(0, T, chunk):
        qkv = F.linear(x[:, s:s + chunk], weight)
        if s == 0:
            out = ops.diff_attention(qkv, coef, H, N, hs)
            buf[:, :qkv.shape[1]].copy_(qkv[..., nq:])
        else:
            out = kv_cache._extend_rows(qkv, buf, coef, None, H, N, hs, dv, s)
        del qkv, out


def memory_leg():
    B, H, N, hs, T, chunk = 1, 16, 2, 128, 32768, 2048
    dv, C = 2 * hs, 16 * 2 * 128
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (torch.randn(B, T, C, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    weight = (torch.randn(ops.packed_width(H, N, hs, dv), C, device=DEV, generator=g) * C ** -0.5).to(torch.bfloat16)
    buf = torch.empty(B, T, H * N * hs + H * dv, device=DEV, dtype=torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    row = {"case": "memory", "dtype": "bf16", "B": B, "H": H, "head_size": hs, "dv": dv, "n_terms": N, "T": T,
           "chunk": chunk}
    with torch.no_grad():
        for name, c in (("one_shot", T), ("chunked", chunk)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _layer_prefill(x, weight, buf, coef, H, N, hs, dv, c)
            b.record()
            b.synchronize()
            row[name + "_peak_extra_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            row[name + "_ms_single_run"] = round(a.elapsed_time(b), 2)
    row["resident_MiB"] = round(base / 2 ** 20, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for row in timing_legs(max(20, args.repeats), args.warmup):
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows.append(memory_leg())
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
