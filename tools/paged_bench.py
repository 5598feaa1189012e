"""Time the paged-cache kernels (``ops.diff_attention_decode_paged``,
``ops.diff_attention_extend_paged``) against the ragged kernels on the contiguous cache,
and count the cache bytes a paged batch holds.

Shape and method are tools/ragged_bench.py's: the cfg2 head shape (H=16, hs=64, dv=128,
N=2, bf16), B=8, t_cap=4096, HIP events in one process, the arms interleaved round-robin
(every repeat runs every arm once), median / min / max of the repeats after warm-up, each
timed window ``inner`` back-to-back calls, reported per call.
  decode (lengths spread evenly from 512 to 4096), per page size P in 64, 256:
    ragged            the ragged decode on the contiguous (B, t_cap) cache
    paged_identity    the same rows cut into pages that lie in order in the pool
    paged_shuffled    the pages permuted across the whole pool
    ragged_again      the ragged arm a second time: the spread between its two copies
                      is the noise band the paged ratios are read against
  extend (Tq=64, positions spread evenly from 448 to 4032), P = 64:
    extend_ragged against extend_paged (shuffled), extend_ragged_again as the band
  cache bytes (computed, not timed), per layer for that batch:
    pages in use x P x W against the ragged cache's B x (block_size + 1) x W, and for
    n_samples = 4 of one 1024-token prompt the pages in use with ``fork`` against without
Every paged arm is checked bitwise against the ragged one before it is timed.
Usage: python tools/paged_bench.py [--out FILE] [--repeats 50] [--warmup 10] [--inner 20]
-> one JSON line per case (also written to FILE as a JSON list)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from differential_transformer_replication_amd import ops  # noqa: E402
from differential_transformer_replication_amd.kv_cache import PagedKVCache  # noqa: E402
from ragged_bench import interleaved_ms, _report  # noqa: E402

DEV = "cuda"
B, H, N, HS, CAP = 8, 16, 2, 64, 4096
DV = 2 * HS
NQ = H * N * HS


def _cache(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = NQ + H * DV
    rows = torch.randn(B, CAP, W, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(B, 64, H, N, HS, device=DEV, generator=g).to(torch.bfloat16)
    return rows, q


def _views(buf):
    return buf[..., :NQ].unflatten(-1, (H, N, HS)), buf[..., NQ:].unflatten(-1, (H, DV))


def _pool(rows, P, shuffled):
    """The contiguous cache cut into pages, in order or permuted across the whole pool."""
    n_pages = B * CAP // P
    pages = rows.view(n_pages, P, -1)
    if not shuffled:
        return pages.clone(), torch.arange(n_pages, dtype=torch.int32, device=DEV).view(B, CAP // P)
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(P)).to(DEV)
    pool = torch.empty_like(pages)
    pool[perm] = pages
    return pool, perm.view(B, CAP // P).to(torch.int32)


def decode_case(P, repeats, warmup, inner):
    rows, q = _cache(0)
    q1 = q[:, 0]
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    host = [512 + (CAP - 512) * b // (B - 1) for b in range(B)]
    lengths = torch.tensor(host, dtype=torch.int32, device=DEV)
    k, v = _views(rows)
    pool_i, tab_i = _pool(rows, P, False)
    pool_s, tab_s = _pool(rows, P, True)
    (ki, vi), (ks, vs) = _views(pool_i), _views(pool_s)
    want = ops.diff_attention_decode_ragged(q1, k, v, coef, lengths)
    row = {"case": "decode", "page_size": P, "dtype": "bf16", "B": B, "H": H, "head_size": HS, "dv": DV, "n_terms": N,
           "t_cap": CAP, "lengths": host, "repeats": repeats, "warmup": warmup, "inner": inner,
           "bytes_per_contiguous_run": P * (NQ + H * DV) * 2,
           "identity_equals_ragged": bool(torch.equal(ops.diff_attention_decode_paged(q1, ki, vi, coef, tab_i, lengths), want)),
           "shuffled_equals_ragged": bool(torch.equal(ops.diff_attention_decode_paged(q1, ks, vs, coef, tab_s, lengths), want))}
    arms = {
        "ragged": lambda: ops.diff_attention_decode_ragged(q1, k, v, coef, lengths),
        "paged_identity": lambda: ops.diff_attention_decode_paged(q1, ki, vi, coef, tab_i, lengths),
        "paged_shuffled": lambda: ops.diff_attention_decode_paged(q1, ks, vs, coef, tab_s, lengths),
        "ragged_again": lambda: ops.diff_attention_decode_ragged(q1, k, v, coef, lengths),
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    for name in ("paged_identity", "paged_shuffled", "ragged_again"):
        row[name + "_over_ragged"] = round(row[name + "_ms"] / row["ragged_ms"], 4)
    return row


def extend_case(P, repeats, warmup, inner):
    Tq = 64
    rows, q = _cache(1)
    coef = torch.tensor([[1.0, -0.6]] * H, device=DEV)
    host = [448 + (CAP - Tq - 448) * b // (B - 1) for b in range(B)]
    pos = torch.tensor(host, dtype=torch.int32, device=DEV)
    k, v = _views(rows)
    pool_s, tab_s = _pool(rows, P, True)
    ks, vs = _views(pool_s)
    want = ops.diff_attention_extend_ragged(q, k, v, coef, pos)
    row = {"case": "extend", "page_size": P, "dtype": "bf16", "B": B, "H": H, "head_size": HS, "dv": DV, "n_terms": N,
           "t_cap": CAP, "Tq": Tq, "pos": host, "repeats": repeats, "warmup": warmup, "inner": inner,
           "shuffled_equals_ragged": bool(torch.equal(ops.diff_attention_extend_paged(q, ks, vs, coef, tab_s, pos), want))}
    arms = {
        "extend_ragged": lambda: ops.diff_attention_extend_ragged(q, k, v, coef, pos),
        "extend_paged": lambda: ops.diff_attention_extend_paged(q, ks, vs, coef, tab_s, pos),
        "extend_ragged_again": lambda: ops.diff_attention_extend_ragged(q, k, v, coef, pos),
    }
    _report(row, interleaved_ms(arms, repeats, warmup, inner))
    for name in ("extend_paged", "extend_ragged_again"):
        row[name + "_over_ragged"] = round(row[name + "_ms"] / row["extend_ragged_ms"], 4)
    return row


def bytes_case():
    """Cache bytes per layer (bf16 rows of W = H*N*hs + H*dv elements); host arithmetic
    through the allocator itself, nothing is launched."""
    W, es = NQ + H * DV, 2
    host = [512 + (CAP - 512) * b // (B - 1) for b in range(B)]
    row = {"case": "cache_bytes", "dtype": "bf16", "row_bytes": W * es, "block_size": CAP, "lengths": host,
           "ragged_bytes": B * (CAP + 1) * W * es}
    for P in (64, 256):
        pages = sum(-(-n // P) for n in host)
        row[f"paged_P{P}_pages"] = pages
        row[f"paged_P{P}_bytes"] = pages * P * W * es
        row[f"paged_P{P}_over_ragged"] = round(pages * P / (B * (CAP + 1)), 4)
    # four samples of one 1024-token prompt, 256 new tokens each, P = 64
    P, prompt, new, n = 64, 1024, 256, 4
    end = prompt + new - 1
    cache = PagedKVCache(n * -(-end // P), P)
    cache._ensure(CAP, "cpu")
    root = cache._new_seq([cache.free.pop() for _ in range(cache._need(prompt))], prompt)
    for pg in cache.pages[root]:
        cache.refcount[pg] = 1
    seqs = [root] + [cache.fork(root) for _ in range(n - 1)]
    row["fork_pages_after_prefill"] = cache.pages_in_use()
    cache._prepare_writes(seqs, [end] * n)
    row.update({"fork_case": {"n_samples": n, "prompt": prompt, "new_tokens": new, "page_size": P},
                "fork_pages": cache.pages_in_use(), "no_fork_pages": n * -(-end // P),
                "fork_over_no_fork": round(cache.pages_in_use() / (n * -(-end // P)), 4)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paged_bench needs the GPU: there is nothing to time without one")
    rows = []
    for case in (lambda: decode_case(64, args.repeats, args.warmup, args.inner),
                 lambda: decode_case(256, args.repeats, args.warmup, args.inner),
                 lambda: extend_case(64, args.repeats, args.warmup, args.inner), bytes_case):
        rows.append(case())
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
