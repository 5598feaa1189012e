"""Time the fp8 (e4m3fn) paged cache against the bf16 paged cache and report what the
quantisation costs in quality.

Method of tools/paged_bench.py: one process, HIP events around ``inner`` back-to-back
calls, ``repeats`` windows after ``warmup`` rounds, the arms taking turns inside every
repeat, median [min, max] per call.  bf16 q, B=8, H=16, hs=64, dv=128, N=2, P=64, the
pages permuted across the whole pool.
  decode, lengths 512 .. 4096 at t_cap 4096 (paged_bench's shape) and all 32768 at t_cap 32768:
    bf16         ops.diff_attention_decode_paged
    bf16_again   the same arm a second time: the band the fp8 ratio is read against
    fp8          ops.diff_attention_decode_paged_fp8 on the same rows, quantised
  write, 8 rows (one decode step) and a 1024-row prefill:
    index_put    the scatter of the bf16 rows the fp8 write replaces
    index_put_again
    quant        ops.kv_quant_rows
  bytes (computed): per (row, head) N*hs + dv + 4*(N+1) against 2*(N*hs + dv).
  quality, a seeded DiffTransformer (bf16): cache bytes held per layer in both formats,
  and, teacher-forced on the unquantised run's greedy tokens, the largest |logit
  difference| and the share of equal greedy tokens over 64 decode steps.
  extend (--extend-only: this leg alone, its own file), Tq in 4, 16, 64, 256 new rows per sequence
  on top of 512 .. 4096 cached ones, all B sequences at the same length, t_cap 4352:
    fp8_extend   ops.diff_attention_extend_paged_fp8, one launch
    fp8_per_row  the per-row loop it replaces (kv_cache._decode_per_row over
                 ops.diff_attention_decode_paged_fp8: PagedKVCache's default on fp8 pages), Tq launches
    bf16_extend  ops.diff_attention_extend_paged on a bf16 pool of the same rows
    The per-row loop costs Tq times a decode step, so a window holds ``inner * 4 // Tq`` (at least 1) calls.
The fp8 arm is checked against the dequantised rows' bf16-cache result before it is timed.
Usage: python tools/fp8_bench.py [--out profiles/fp8_bench.json] [--repeats 50] [--warmup 10]
       [--inner 20] [--skip-long] [--skip-quality]
       python tools/fp8_bench.py --extend-only --out profiles/fp8_extend_bench.json
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
B, H, N, HS, P = 8, 16, 2, 64, 64
DV = 2 * HS
NQ = H * N * HS
W = NQ + H * DV


def _views(buf):
    return buf[..., :NQ].unflatten(-1, (H, N, HS)), buf[..., NQ:].unflatten(-1, (H, DV))


def _pools(cap, seed):
    """A shuffled bf16 pool of B * cap / P pages, the same rows quantised, and the table."""
    n_pages = B * cap // P
    g = torch.Generator(device=DEV).manual_seed(seed)
    pool = torch.empty(n_pages, P, W, device=DEV, dtype=torch.bfloat16)
    pool8 = torch.empty(n_pages, P, W, device=DEV, dtype=torch.uint8)
    scales = torch.empty(n_pages, P, H, N + 1, device=DEV, dtype=torch.float32)
    step = max(1, n_pages // 16)
    for s in range(0, n_pages, step):                      # in slices: the fp32 temporaries stay small
        rows = torch.randn(min(step, n_pages - s), P, W, device=DEV, generator=g).to(torch.bfloat16)
        pool[s:s + step] = rows
        k, v = _views(rows)
        kb, ks = ops.kv_quant_reference(k)
        vb, vs = ops.kv_quant_reference(v)
        pool8[s:s + step, :, :NQ] = kb.flatten(2)
        pool8[s:s + step, :, NQ:] = vb.flatten(2)
        scales[s:s + step, ..., :N] = ks
        scales[s:s + step, ..., N] = vs
    table = torch.randperm(n_pages, generator=torch.Generator().manual_seed(P + cap)).to(DEV).view(B, cap // P).to(torch.int32)
    return pool, pool8, scales, table.contiguous()


def decode_case(cap, host, repeats, warmup, inner):
    pool, pool8, scales, table = _pools(cap, cap)
    q = torch.randn(B, H, N, HS, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    lengths = torch.tensor(host, dtype=torch.int32, device=DEV)
    k, v = _views(pool)
    k8, v8 = _views(pool8)
    got = ops.diff_attention_decode_paged_fp8(q, k8, v8, scales, coef, table, lengths).float()
    # the reference for the check: the bf16 kernel on the dequantised rows, rounded to bf16
    deq = torch.empty_like(pool)
    dk, dv_ = _views(deq)
    dk.copy_(k8.view(torch.float8_e4m3fn).float() * scales[..., :N, None])
    dv_.copy_(v8.view(torch.float8_e4m3fn).float() * scales[..., N, None])
    want = ops.diff_attention_decode_paged(q, dk, dv_, coef, table, lengths).float()
    del deq
    rel = ((got - want).abs().max() / want.abs().max()).item()
    rows = sum(host)
    row = {"case": "decode", "page_size": P, "q_dtype": "bf16", "B": B, "H": H, "head_size": HS, "dv": DV, "n_terms": N,
           "t_cap": cap, "lengths": host if len(set(host)) > 1 else host[0], "repeats": repeats, "warmup": warmup,
           "inner": inner, "bytes_per_row_head": {"bf16": 2 * (N * HS + DV), "fp8": N * HS + DV + 4 * (N + 1)},
           "bytes_ratio": round((N * HS + DV + 4 * (N + 1)) / (2 * (N * HS + DV)), 4),
           "bf16_cache_bytes_read": rows * H * 2 * (N * HS + DV), "fp8_cache_bytes_read": rows * H * (N * HS + DV + 4 * (N + 1)),
           "fp8_vs_bf16_on_dequantised_rows_rel_err": rel}
    assert rel <= 2e-2, rel
    arms = {
        "bf16": lambda: ops.diff_attention_decode_paged(q, k, v, coef, table, lengths),
        "fp8": lambda: ops.diff_attention_decode_paged_fp8(q, k8, v8, scales, coef, table, lengths),
        "bf16_again": lambda: ops.diff_attention_decode_paged(q, k, v, coef, table, lengths),
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    row["fp8_over_bf16"] = round(row["fp8_ms"] / row["bf16_ms"], 4)
    row["bf16_again_over_bf16"] = round(row["bf16_again_ms"] / row["bf16_ms"], 4)
    row["bf16_GBps"] = round(row["bf16_cache_bytes_read"] / row["bf16_ms"] / 1e6, 1)
    row["fp8_GBps"] = round(row["fp8_cache_bytes_read"] / row["fp8_ms"] / 1e6, 1)
    row["fp8_faster_than_the_band"] = bool(row["fp8_ms"] < min(row["bf16_ms"], row["bf16_again_ms"])
                                           - abs(row["bf16_ms"] - row["bf16_again_ms"]))
    return row


EXTEND_CAP = 4096 + 256                       # the longest cached length and the most new rows
EXTEND_TQ = (4, 16, 64, 256)
EXTEND_LENGTHS = (512, 1024, 2048, 4096)


def extend_cases(repeats, warmup, inner):
    """One row per (cached length, Tq); the pools are made once."""
    pool, pool8, scales, table = _pools(EXTEND_CAP, 11)
    k, v = _views(pool)
    k8, v8 = _views(pool8)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    deq = torch.empty_like(pool)                  # the reference for the check: the bf16 kernel on the dequantised rows
    dk, dv_ = _views(deq)
    dk.copy_(k8.view(torch.float8_e4m3fn).float() * scales[..., :N, None])
    dv_.copy_(v8.view(torch.float8_e4m3fn).float() * scales[..., N, None])
    g = torch.Generator(device=DEV).manual_seed(2)
    for L in EXTEND_LENGTHS:
        pos = torch.full((B,), L, dtype=torch.int32, device=DEV)
        for Tq in EXTEND_TQ:
            q = torch.randn(B, Tq, H, N, HS, device=DEV, generator=g).to(torch.bfloat16)

            def per_row():
                return kv_cache._decode_per_row(
                    lambda i, n: ops.diff_attention_decode_paged_fp8(q[:, i], k8, v8, scales, coef, table, n), Tq, pos,
                    torch.full_like(pos, Tq))

            got = ops.diff_attention_extend_paged_fp8(q, k8, v8, scales, coef, table, pos).float()
            want = ops.diff_attention_extend_paged(q, dk, dv_, coef, table, pos).float()
            rel = ((got - want).abs().max() / want.abs().max()).item()
            rel_rows = ((got - per_row().float()).abs().max() / want.abs().max()).item()
            assert rel <= 2e-2 and rel_rows <= 2e-2, (L, Tq, rel, rel_rows)
            n_in = max(1, inner * 4 // Tq)
            # bytes the cache rows contribute, per format: every (sequence, head) reads rows 0 .. L + Tq - 1 twice
            # in the extend kernels (two passes; pass 1 K only) and once per new row in the per-row loop
            row = {"case": "extend", "page_size": P, "q_dtype": "bf16", "B": B, "H": H, "head_size": HS, "dv": DV,
                   "n_terms": N, "t_cap": EXTEND_CAP, "cached": L, "Tq": Tq, "repeats": repeats, "warmup": warmup,
                   "inner": n_in, "fp8_extend_vs_bf16_on_dequantised_rows_rel_err": rel,
                   "fp8_extend_vs_fp8_per_row_rel_err": rel_rows}
            arms = {
                "fp8_extend": lambda: ops.diff_attention_extend_paged_fp8(q, k8, v8, scales, coef, table, pos),
                "fp8_per_row": per_row,
                "bf16_extend": lambda: ops.diff_attention_extend_paged(q, k, v, coef, table, pos),
            }
            _report(row, interleaved_ms(arms, repeats, warmup, n_in))
            row["fp8_extend_over_fp8_per_row"] = round(row["fp8_extend_ms"] / row["fp8_per_row_ms"], 4)
            row["fp8_extend_over_bf16_extend"] = round(row["fp8_extend_ms"] / row["bf16_extend_ms"], 4)
            row["per_row_wins"] = bool(row["fp8_per_row_ms"] < row["fp8_extend_ms"])
            yield row


def write_case(Bw, Tn, repeats, warmup, inner):
    n_pages = max(Bw * Tn // P, 1) + 3
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(Bw, Tn, NQ + W, device=DEV, generator=g).to(torch.bfloat16)
    new_rows = qkv[..., NQ:]
    k_new = qkv[..., NQ:2 * NQ].unflatten(-1, (H, N, HS))
    v_new = qkv[..., 2 * NQ:].unflatten(-1, (H, DV))
    pool = torch.zeros(n_pages + 1, P, W, device=DEV, dtype=torch.bfloat16)
    pool8 = torch.zeros(n_pages + 1, P, W, device=DEV, dtype=torch.uint8)
    scales = torch.zeros(n_pages + 1, P, H, N + 1, device=DEV)
    at = torch.randperm(n_pages * P, generator=torch.Generator().manual_seed(8))[:Bw * Tn].to(DEV).view(Bw, Tn)
    page, r = at // P, at % P
    slots = at.to(torch.int32).flatten().contiguous()
    k8, v8 = _views(pool8)
    row = {"case": "write", "rows": Bw * Tn, "B": Bw, "Tn": Tn, "page_size": P, "dtype": "bf16", "H": H, "head_size": HS,
           "dv": DV, "n_terms": N, "repeats": repeats, "warmup": warmup, "inner": inner}
    arms = {
        "index_put": lambda: pool.index_put_((page, r), new_rows),
        "quant": lambda: ops.kv_quant_rows(k_new, v_new, k8, v8, scales, slots),
        "index_put_again": lambda: pool.index_put_((page, r), new_rows),
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    row["quant_over_index_put"] = round(row["quant_ms"] / row["index_put_ms"], 4)
    row["index_put_again_over_index_put"] = round(row["index_put_again_ms"] / row["index_put_ms"], 4)
    return row


@torch.no_grad()
def quality_case(steps=64):
    torch.manual_seed(0)
    model = D.DiffTransformer(vocab_size=512, n_embd=512, n_head=4, n_layer=4, block_size=512, dropout=0.0)
    model = model.to(DEV).to(torch.bfloat16).eval()
    for p in model.parameters():              # non-zero lambdas so the two branches differ
        if p.dim() == 1 and p.shape[0] == 64:
            torch.nn.init.normal_(p, std=0.1)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in (100, 200, 300, 37)]
    need = sum(-(-(p.shape[0] + steps) // P) for p in prompts)
    plain, fp8 = kv_cache.PagedKVCache(need, P), kv_cache.PagedKVCache(need, P, kv_dtype="fp8_e4m3")
    ids, logits = kv_cache.prefill_paged(model, prompts, plain)
    ids8, logits8 = kv_cache.prefill_paged(model, prompts, fp8)
    worst, equal, total, ref_mag = 0.0, 0, 0, 0.0
    for _ in range(steps):
        tok = logits.argmax(-1, keepdim=True)                 # the unquantised run's greedy token feeds both
        logits = kv_cache.decode_paged(model, ids, tok, plain)
        logits8 = kv_cache.decode_paged(model, ids8, tok, fp8)
        worst = max(worst, (logits.float() - logits8.float()).abs().max().item())
        ref_mag = max(ref_mag, logits.float().abs().max().item())
        equal += int((logits.argmax(-1) == logits8.argmax(-1)).sum())
        total += len(prompts)
    per_layer = lambda c: c.cache_bytes() // len(c.pool)      # noqa: E731
    return {"case": "quality", "model": "DiffTransformer(vocab 512, n_embd 512, n_head 4, n_layer 4, block 512), bf16, seed 0",
            "prompts": [p.shape[0] for p in prompts], "decode_steps": steps, "page_size": P,
            "cache_bytes_per_layer": {"bf16": per_layer(plain), "fp8_e4m3": per_layer(fp8)},
            "cache_bytes_ratio": round(per_layer(fp8) / per_layer(plain), 4),
            "max_abs_logit_difference": round(worst, 5), "max_abs_logit": round(ref_mag, 5),
            "equal_greedy_tokens": equal, "greedy_tokens": total, "equal_greedy_share": round(equal / total, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--extend-only", action="store_true", help="the multi-row (extend) leg alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_bench needs the GPU: there is nothing to time without one")
    if not ops.fp8_cache_supported():
        raise SystemExit("the built library has no fp8-cache entry points")
    r = (args.repeats, args.warmup, args.inner)
    if args.extend_only:
        if not ops.extend_fp8_supported(torch.bfloat16, HS, N, DV):
            raise SystemExit("the built library has no fp8 extend plan for this shape")
        rows = []
        for row in extend_cases(*r):
            rows.append(row)
            print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(rows, fh, indent=1)
                fh.write("\n")
        return
    cases = [lambda: decode_case(4096, [512 + (4096 - 512) * b // (B - 1) for b in range(B)], *r)]
    if not args.skip_long:
        cases.append(lambda: decode_case(32768, [32768] * B, *r))
    cases += [lambda: write_case(8, 1, *r), lambda: write_case(1, 1024, *r)]
    if not args.skip_quality:
        cases.append(quality_case)
    rows = []
    for case in cases:
        rows.append(case())
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")
    long_rows = [x for x in rows if x["case"] == "decode" and x["t_cap"] == 32768]
    if long_rows and not long_rows[0]["fp8_faster_than_the_band"]:
        raise SystemExit("fp8 decode at L = 32768 is not faster than bf16 by more than the bf16 / bf16_again band")


if __name__ == "__main__":
    main()
