"""Time the shared-prefix decode against the per-sequence paged decode it can replace.

Method of tools/decode_rows_bench.py: one process, HIP events around ``inner`` back-to-back
calls, ``repeats`` windows after ``warmup`` rounds, the arms taking turns inside every repeat,
median [min, max] per call.  bf16 q, H=16, hs=64, dv=128, N=2, pages of 64 shuffled over the
pool; 4 prompts of 512 .. 4096 shared rows, k in 2, 4, 8 samples of each (B = 4k, sample-major
within a prompt, as ``generate_paged(n_samples=k)`` lays them out), every sample with a short
tail of its own (40 + 3b rows); a bf16 pool and an fp8 pool.
  shared   ops.diff_attention_decode_paged_shared(_fp8): group pass + one-row pass + combine
  paged    ops.diff_attention_decode_paged(_fp8) on the same pool, table and lengths
``shared`` is checked bitwise against ``paged`` before it is timed.  Bytes: the cache bytes an arm
reads (scales included on fp8 pages): ``paged`` every row of every sequence, ``shared`` the
covered rows once per group and the rest per sequence.
Usage: python tools/shared_decode_bench.py [--out profiles/shared_decode_bench.json] [--repeats 20]
       [--warmup 10] [--inner 20]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
P = 64
PROMPTS = 4
SAMPLES = (2, 4, 8)
SHARED = (512, 1024, 2048, 4096)
CHUNK = 256


def _case(H, N, hs, L, k, fp8, repeats, warmup, inner, seed):
    dv = 2 * hs
    nq = H * N * hs
    Bn = PROMPTS * k
    tails = [40 + 3 * b for b in range(Bn)]
    lengths = [L + t for t in tails]
    cap = -(-max(lengths) // 256) * 256
    shared_pages, own_pages = L // P, [-(-(L + t) // P) - L // P for t in tails]
    n_pages = PROMPTS * shared_pages + sum(own_pages)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = torch.randn(n_pages, P, nq + H * dv, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(Bn, H, N, hs, device=DEV, generator=g).to(torch.bfloat16)
    coef = torch.tensor([[1.0, -0.6][:N]] * H, device=DEV)
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table, at = torch.full((Bn, cap // P), -1, dtype=torch.int32), PROMPTS * shared_pages
    for b in range(Bn):
        pr = b // k
        ids = perm[pr * shared_pages:(pr + 1) * shared_pages] + perm[at:at + own_pages[b]]
        at += own_pages[b]
        table[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    table = table.to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    plan = ops.shared_decode_plan([tuple(range(pr * k, (pr + 1) * k)) for pr in range(PROMPTS)], [L] * PROMPTS, Bn, DEV)
    views = lambda buf: (buf[..., :nq].unflatten(-1, (H, N, hs)), buf[..., nq:].unflatten(-1, (H, dv)))
    if fp8:
        kk, vv = views(rows)
        kb, ks = ops.kv_quant_reference(kk)
        vb, vs = ops.kv_quant_reference(vv)
        pool8 = torch.cat([kb.flatten(2), vb.flatten(2)], dim=-1).contiguous()
        scales = torch.cat([ks, vs[..., None]], dim=-1).contiguous()
        k8, v8 = views(pool8)
        del rows, kk, vv, kb, vb
        arms = {"shared": lambda: ops.diff_attention_decode_paged_shared_fp8(q, k8, v8, scales, coef, table, ln, plan),
                "paged": lambda: ops.diff_attention_decode_paged_fp8(q, k8, v8, scales, coef, table, ln)}
        row_bytes = N * hs + dv + 4 * (N + 1)
    else:
        kk, vv = views(rows)
        arms = {"shared": lambda: ops.diff_attention_decode_paged_shared(q, kk, vv, coef, table, ln, plan),
                "paged": lambda: ops.diff_attention_decode_paged(q, kk, vv, coef, table, ln)}
        row_bytes = 2 * (N * hs + dv)
    assert torch.equal(arms["shared"](), arms["paged"]()), "shared != paged"
    wide = -(-cap // CHUNK) * H * Bn >= 8192
    chunk = 2 * CHUNK if wide else CHUNK
    covered = L // chunk * chunk
    paged_bytes = H * sum(lengths) * row_bytes
    shared_bytes = H * (PROMPTS * covered + sum(n - covered for n in lengths)) * row_bytes
    row = {"case": "shared_decode", "cache": "fp8_pages_64" if fp8 else "bf16_pages_64", "q_dtype": "bf16", "B": Bn,
           "prompts": PROMPTS, "samples": k, "H": H, "head_size": hs, "dv": dv, "n_terms": N, "t_cap": cap,
           "shared_rows": L, "covered_rows": covered, "chunk": chunk, "own_tail_rows": [tails[0], tails[-1]],
           "repeats": repeats, "warmup": warmup, "inner": inner, "shared_equals_paged_bitwise": True,
           "paged_bytes_read": paged_bytes, "shared_bytes_read": shared_bytes}
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    row["shared_over_paged"] = round(row["shared_ms"] / row["paged_ms"], 4)
    row["bytes_shared_over_paged"] = round(shared_bytes / paged_bytes, 4)
    row["paged_TBps"] = round(paged_bytes / row["paged_ms"] / 1e9, 3)
    row["shared_TBps"] = round(shared_bytes / row["shared_ms"] / 1e9, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    rows = []
    for fp8 in (False, True):
        for L in SHARED:
            for k in SAMPLES:
                rows.append(_case(16, 2, 64, L, k, fp8, a.repeats, a.warmup, a.inner, seed=L + k))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    with open(a.out, "w") as fh:
                        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
