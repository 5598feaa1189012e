// spec_round.hip -- the glue of a fixed-shape speculative round as device code (dta_spec_feed_rows,
// dta_spec_commit_lengths), gfx950.
//
// A round that always runs K + 1 rows per sequence can be captured once and replayed if no host value
// shapes it.  The model step, the sampler and spec.hip's accept + draft kernel already read their
// positions, counts and lengths on the device; these two launches are what was left on the host: the
// round's tokens, counts and sampler offsets before the step, and the cache lengths after it.  The
// definition is include/diffattn.h's ("A fixed-shape speculative round").
//
//   * feed: one thread per (sequence, row j of K + 1).  Each reads its sequence's three scalars, and one
//     token: the pending one (j = 0, live rows only) or draft j - 1 (j <= d only).  Every thread stores its
//     idx and offset entry, padding included; thread j = 0 stores the count.
//   * commit: one thread per sequence, one load-add-store of its own slot (the slots are distinct).
// Integers only, 64-bit address arithmetic, no atomics, no LDS.  Every device-read value is clamped before
// it forms an address: hlen into [0, cap], dcnt into [0, K], a slot into [0, n_slots - 1], m into [0, K + 1].
#include "../../include/diffattn.h"
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void spec_feed_rows_kernel(SpecFeedParams P) {
  const int T = P.K + 1;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)P.B * T) return;
  const int64_t b = i / T;
  const int j = (int)(i - b * T);
  const int L = min(max(P.hlen[b], 0), P.cap);
  const int rem = P.remaining[b];
  const bool live = rem > 0 && L >= 1;
  const int d = live ? min(max(P.dcnt[b], 0), P.K) : 0;
  int tok = 0;
  if (j == 0) {
    if (live) tok = P.hist[b * P.hist_stride + (L - 1)];
    P.counts[b] = live ? d + 1 : 0;
  } else if (j <= d) {
    tok = P.draft[b * P.draft_stride + (j - 1)];
  }
  P.idx[b * P.idx_stride + j] = (int64_t)min(max(tok, 0), P.vocab - 1);
  P.offset[b * P.offset_stride + j] = (int64_t)P.total - (int64_t)rem + j;
}

__global__ __launch_bounds__(kThreads) void spec_commit_lengths_kernel(SpecCommitParams P) {
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= P.B) return;
  int64_t s = b;
  if (P.slots) s = min(max(P.slots[b], (int64_t)0), (int64_t)P.n_slots - 1);
  const int m = min(max(P.result[b * 2], 0), P.K + 1);
  P.lengths[s] = (int)min((int64_t)P.lengths[s] + m, (int64_t)P.t_cap);
}

}  // namespace

int launch_spec_feed(const SpecFeedParams& p, hipStream_t st) {
  if (p.B == 0) return 0;
  const int64_t n = (int64_t)p.B * (p.K + 1);
  hipLaunchKernelGGL(spec_feed_rows_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p);
  return (int)hipGetLastError();
}

int launch_spec_commit(const SpecCommitParams& p, hipStream_t st) {
  if (p.B == 0) return 0;
  hipLaunchKernelGGL(spec_commit_lengths_kernel, dim3((unsigned)(((int64_t)p.B + kThreads - 1) / kThreads)), dim3(kThreads),
                     0, st, p);
  return (int)hipGetLastError();
}

}  // namespace dta
