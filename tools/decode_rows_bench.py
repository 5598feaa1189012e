"""Time the split-key decode for a short multi-row step against the two paths it can replace.

Method of tools/fp8_bench.py --extend-only: one process, HIP events around ``inner``
back-to-back calls, ``repeats`` windows after ``warmup`` rounds, the arms taking turns inside
every repeat, median [min, max] per call.  bf16 q, B=8, H=16, hs=64, dv=128, N=2; Tq in 2, 4, 8
new rows per sequence on top of 512 .. 4096 cached ones, all sequences at the same length;
a contiguous bf16 cache and fp8 pages of 64 (shuffled over the pool); and one long case, B=1,
H=16, hs=128, dv=256, 32768 cached rows, Tq=4.
  rows      ops.diff_attention_decode_rows / _paged_fp8: one split launch, one combine launch
  per_row   kv_cache._decode_per_row over the one-row decode op: Tq launch pairs
  extend    ops.diff_attention_extend_ragged / _paged_fp8: one MFMA launch
  decode1   the one-row decode at the step's last length, for the bandwidth it reaches
``rows`` is checked bitwise against ``per_row`` before it is timed.  Bandwidth: the cache bytes
of rows 0 .. L + Tq - 1 (scales included on fp8 pages), read once, over the time of the call.
Usage: python tools/decode_rows_bench.py [--out profiles/decode_rows_bench.json] [--repeats 20]
       [--warmup 10] [--inner 20] [--skip-long]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops, kv_cache  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
P = 64
TQS = (2, 4, 8)
LENGTHS = (512, 1024, 2048, 4096)


def _case(Bn, H, N, hs, L, Tq, fp8, repeats, warmup, inner, seed):
    dv = 2 * hs
    nq = H * N * hs
    cap = -(-(L + 8) // 256) * 256
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = torch.randn(Bn, cap, nq + H * dv, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(Bn, Tq, H, N, hs, device=DEV, generator=g).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6][:N]] * H, device=DEV)
    pos = torch.full((Bn,), L, dtype=torch.int32, device=DEV)
    last = pos + Tq
    views = lambda buf: (buf[..., :nq].unflatten(-1, (H, N, hs)), buf[..., nq:].unflatten(-1, (H, dv)))
    if fp8:
        n_pages = Bn * cap // P
        k, v = views(rows.view(n_pages, P, -1))
        kb, ks = ops.kv_quant_reference(k)
        vb, vs = ops.kv_quant_reference(v)
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).to(DEV)
        pool8 = torch.empty(n_pages, P, nq + H * dv, device=DEV, dtype=torch.uint8)
        scales = torch.empty(n_pages, P, H, N + 1, device=DEV, dtype=torch.float32)
        pool8[perm] = torch.cat([kb.flatten(2), vb.flatten(2)], dim=-1)
        scales[perm] = torch.cat([ks, vs[..., None]], dim=-1)
        table = perm.view(Bn, cap // P).to(torch.int32).contiguous()
        k8, v8 = views(pool8)
        del rows, k, v, kb, vb
        one = lambda qr, n: ops.diff_attention_decode_paged_fp8(qr, k8, v8, scales, coef, table, n)
        arms = {"rows": lambda: ops.diff_attention_decode_rows_paged_fp8(q, k8, v8, scales, coef, table, pos),
                "extend": lambda: ops.diff_attention_extend_paged_fp8(q, k8, v8, scales, coef, table, pos)}
        row_bytes = N * hs + dv + 4 * (N + 1)
    else:
        k, v = views(rows)
        one = lambda qr, n: ops.diff_attention_decode_ragged(qr, k, v, coef, n)
        arms = {"rows": lambda: ops.diff_attention_decode_rows(q, k, v, coef, pos),
                "extend": lambda: ops.diff_attention_extend_ragged(q, k, v, coef, pos)}
        row_bytes = 2 * (N * hs + dv)
    arms["per_row"] = lambda: kv_cache._decode_per_row(lambda i, n: one(q[:, i], n), Tq, pos, torch.full_like(pos, Tq))
    arms["decode1"] = lambda: one(q[:, Tq - 1], last)
    got, want = arms["rows"](), arms["per_row"]()
    assert torch.equal(got, want), "rows != per-row loop"
    rel = ((got.float() - arms["extend"]().float()).abs().max() / want.float().abs().max()).item()
    assert rel <= 2e-2, rel
    n_in = max(1, inner * 2 // Tq)
    cache_bytes = Bn * H * (L + Tq) * row_bytes
    row = {"case": "decode_rows", "cache": "fp8_pages_64" if fp8 else "bf16_contiguous", "q_dtype": "bf16", "B": Bn, "H": H,
           "head_size": hs, "dv": dv, "n_terms": N, "t_cap": cap, "cached": L, "Tq": Tq, "repeats": repeats,
           "warmup": warmup, "inner": n_in, "rows_equal_per_row_bitwise": True, "rows_vs_extend_rel_err": rel,
           "cache_bytes_read_once": cache_bytes}
    _report(row, interleaved_ms(arms, repeats, warmup, n_in))
    row["rows_over_per_row"] = round(row["rows_ms"] / row["per_row_ms"], 4)
    row["rows_over_extend"] = round(row["rows_ms"] / row["extend_ms"], 4)
    row["rows_over_decode1"] = round(row["rows_ms"] / row["decode1_ms"], 4)
    row["rows_TBps"] = round(cache_bytes / row["rows_ms"] / 1e9, 3)
    row["decode1_TBps"] = round(cache_bytes / row["decode1_ms"] / 1e9, 3)
    row["rows_share_of_decode1_bandwidth"] = round(row["rows_TBps"] / row["decode1_TBps"], 4)
    row["fastest"] = min(("rows", "per_row", "extend"), key=lambda a: row[a + "_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rows, fh, indent=1)

    for fp8 in (False, True):
        for L in LENGTHS:
            for Tq in TQS:
                emit(_case(8, 16, 2, 64, L, Tq, fp8, a.repeats, a.warmup, a.inner, seed=L + Tq))
    if not a.skip_long:
        for fp8 in (False, True):
            emit(_case(1, 16, 2, 128, 32768, 4, fp8, a.repeats, a.warmup, a.inner, seed=7))


if __name__ == "__main__":
    main()
