// spec.hip -- one round of prompt-lookup speculative decoding on the device (dta_spec_accept_draft), gfx950.
//
// One 256-thread workgroup per sequence, one launch per round: the acceptance of the round's sampled
// rows against the draft they verified, the append of what was emitted to the sequence's history, and
// the next draft by n-gram lookup in that history.  The definition is include/diffattn.h's
// ("Speculative decoding"); what this file adds is the shape of the work.
//
//   * Accept is at most 8 rows: every thread computes (a, m, stop) for itself from the same loads
//     (statically unrolled, so nothing is indexed in registers), thread j < m stores emitted token j.
//   * The history a round reads is the one it has just extended.  No load depends on a store of this
//     launch: position p of the new history is hist[p] below the old length and tok[p - old length]
//     from there on (at()), so no barrier orders the append against the lookup.
//   * Lookup: thread i owns the ends e = ngram_min - 1 + i, + 256, ...; mu(e) is a run of at most 8
//     compares against the suffix held in registers, entered only where the last token matches.  The
//     winner is the integer maximum of (mu << 32 | e) -- longest, then latest -- over the thread's
//     ends, the 64 lanes (xor butterfly) and the 4 waves (LDS), as sample.hip's (key, ~index).
//   * Thread 0 stores the sequence's scalars after the workgroup's one barrier, which every wave
//     reaches only after it has read them.
// Integers only: no floating point, no atomics, no dependence on B, on the row's index or on timing.
// Every device-read value is clamped before it forms an address: hlen into [0, cap], dcnt into
// [0, min(K, Tn - 1)], remaining <= 0 is a finished row, and m is cut to the room left in hist.
#include "../../include/diffattn.h"
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 8;                       // K + 1 <= 8 rows a round, n-grams of at most 8 tokens

__global__ __launch_bounds__(kThreads) void spec_accept_draft_kernel(SpecParams P) {
  __shared__ unsigned long long red64[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t b = blockIdx.x;
  int* res = P.result + b * 2;
  const int rem0 = P.remaining[b];
  if (rem0 <= 0) {                             // finished: nothing of the row's state is touched
    if (tid == 0) { res[0] = 0; res[1] = 0; }
    return;
  }
  int* hist = P.hist + b * P.hist_stride;
  int* draft = P.draft + b * P.draft_stride;
  const int64_t* tok = P.tok + b * P.tok_stride;
  const int L0 = min(max(P.hlen[b], 0), P.cap);
  const int dc = min(max(P.dcnt[b], 0), min(P.K, max(P.Tn - 1, 0)));

  // ---- accept
  int a = 0;
  bool run = true;
#pragma unroll
  for (int j = 0; j < kRows - 1; ++j) {
    if (j < dc) {
      run = run && tok[j] == (int64_t)draft[j];
      a += run;
    }
  }
  int m = min(min(a + 1, rem0), min(P.Tn, P.cap - L0));
  bool stop = false;
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    if (j < m && !stop) {
      const int64_t t = tok[j];
      if (t < 0 || t == (int64_t)P.eos) { m = j + 1; stop = true; }
    }
  }
  const int rem = stop ? 0 : rem0 - m;
  const int L = L0 + m;
  if (tid < m) hist[L0 + tid] = (int)tok[tid];
  auto at = [&](int p) { return p >= L0 ? (int)tok[p - L0] : hist[p]; };     // 0 <= p < L

  // ---- draft
  const bool look = P.nmin >= 1 && rem > 1 && L > P.nmin;
  unsigned long long best = 0;
  if (look) {
    int suf[kRows];
#pragma unroll
    for (int t = 0; t < kRows; ++t) suf[t] = (t < P.nmax && L - 1 - t >= 0) ? at(L - 1 - t) : 0;
    for (int e = P.nmin - 1 + tid; e < L - 1; e += kThreads) {
      if (at(e) != suf[0]) continue;
      int n = 1;
      bool same = true;
#pragma unroll
      for (int t = 1; t < kRows; ++t) {
        if (t < P.nmax && t <= e && same) {
          same = at(e - t) == suf[t];
          n += same;
        }
      }
      if (n >= P.nmin) {
        const unsigned long long key = ((unsigned long long)n << 32) | (uint32_t)e;
        best = key > best ? key : best;
      }
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), d), lo = __shfl_xor((uint32_t)best, d);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o > best ? o : best;
  }
  if (lane == 0) red64[wid] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) best = red64[w] > best ? red64[w] : best;
  int nd = 0;
  if (best != 0) {
    const int e = (int)(uint32_t)best;
    nd = max(min(min(P.K, L - 1 - e), min(rem - 1, P.t_cap - L)), 0);
    if (tid < nd) draft[tid] = at(e + 1 + tid);
  }
  if (tid == 0) {
    P.hlen[b] = L;
    P.remaining[b] = rem;
    P.dcnt[b] = nd;
    res[0] = m;
    res[1] = nd;
  }
}

}  // namespace

int launch_spec(const SpecParams& p, hipStream_t st) {
  if (p.B == 0) return 0;
  hipLaunchKernelGGL(spec_accept_draft_kernel, dim3((unsigned)p.B), dim3(kThreads), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace dta
