// penalty.hip -- repetition / frequency / presence penalties, logit bias and the min-p floor of logits rows
// (dta_penalize_rows), gfx950.
//
// One 256-thread workgroup per logits row, one fp32 output row per workgroup; dta_sample_rows then reads
// that row as an fp32 input.  The definition is include/diffattn.h's ("Sampling penalties"); what this
// file adds is the shape of the work.
//
//   * The row's context -- its sequence's history and the first min(j, dcnt) drafted tokens -- is
//     counted into a table of V 32-bit entries: bit 31 is "seen at a position before gen_start", the
//     low 31 bits count the occurrences at and after it (cap + K < 2^31, so the count never reaches
//     the flag).  s_i is entry != 0, c_i the low bits.  The table is zeroed by the workgroup, filled
//     with integer or / add atomics (they commute: the entries do not depend on the order the context
//     is walked in) and read after a barrier.  It lives in LDS for V <= kLdsMaxV, and in the row's own
//     slice of the caller's workspace beyond that (every entry is zeroed first: nothing is assumed of
//     the workspace; the table loads bypass the L1 the atomics do not pass through).  A row with an
//     empty context skips the table.
//   * Element i of a row belongs to chunk i / 4 and chunk c to thread c % 256 in round c / 256, whichever
//     way it is loaded or stored (one 8- or 16-byte access where the row starts aligned to it, element
//     accesses otherwise).  Every element is computed alone, so nothing depends on that choice.
//   * Steps 1 - 3 are one pass that stores the row and keeps each thread's maximum as the order-preserving
//     integer image of the float; the workgroup's maximum is an integer max (shuffles, then LDS).  The
//     floor is a second pass in which a thread re-reads the elements it stored itself and overwrites
//     those below m + gap with -inf.
// Floating-point contraction is off for this file: each operation of the definition is one rounding.
// -fno-honor-nans is in force for this library, so every NaN test here is on the bits.  No
// floating-point atomics; every address is 64-bit arithmetic on clamped values.
#include "../../include/diffattn.h"
#include "dta_common.h"
#include "dta_internal.h"

#pragma clang fp contract(off)

namespace dta {

namespace {

constexpr int kThreads = 256;
constexpr int kLdsMaxV = DTA_PENALTY_LDS_MAX_V;        // 4 * V bytes of LDS beside the 16 static ones
constexpr uint32_t kSeen = 0x80000000u;
static_assert(kLdsMaxV % 4 == 0 && (size_t)kLdsMaxV * 4 + 64 <= 160 * 1024, "the table and the static LDS fit one CU");

__device__ __forceinline__ uint32_t okey(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ bool nan_bits(float x) { return (__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// 4 consecutive elements of a row; vec: the row starts on a multiple of 4 elements' bytes
template <class E>
__device__ __forceinline__ void load4(const E* p, bool vec, int n, float* x) {
  if (vec && n == 4) {
    typedef E v4 __attribute__((ext_vector_type(4)));
    const v4 v = *reinterpret_cast<const v4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = (float)v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < n ? (float)p[j] : 0.f;
  }
}

template <class E, bool LDS>
__global__ __launch_bounds__(kThreads) void penalize_rows_kernel(PenaltyParams P) {
  extern __shared__ uint32_t lds_tbl[];
  __shared__ uint32_t redu[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t r = blockIdx.x;
  const int64_t b = r / P.Tn;
  const int j = (int)(r - b * P.Tn);
  const int V = P.V;

  const int L = min(max(P.hlen[b], 0), P.cap);
  const int g = min(max(P.gen_start ? P.gen_start[b] : 0, 0), L);
  const int d = P.draft ? min(max(P.dcnt[b], 0), P.K) : 0;
  const int e = min(j, d);
  const float theta = P.theta_dev ? P.theta_dev[b] : P.theta;
  const float fr = P.freq_dev ? P.freq_dev[b] : P.freq;
  const float pr = P.pres_dev ? P.pres_dev[b] : P.pres;
  const float gap = P.gap_dev ? P.gap_dev[b] : P.gap;
  const bool rep_on = !nan_bits(theta) && theta != 1.f;
  const bool cnt_on = !nan_bits(fr) && !nan_bits(pr);
  const bool floor_on = finite_bits(gap) && gap < 0.f;
  const bool ctx = L + e > 0;

  uint32_t* tbl = lds_tbl;
  if constexpr (!LDS) tbl = P.ws + r * (int64_t)V;

  // ---- the row's table: zero, count, and a barrier before it is read
  if (ctx) {
    if constexpr (LDS) {
      typedef uint32_t u4 __attribute__((ext_vector_type(4)));
      for (int c = tid; c < (V + 3) >> 2; c += kThreads) reinterpret_cast<u4*>(tbl)[c] = u4{0u, 0u, 0u, 0u};
    } else {
      for (int i = tid; i < V; i += kThreads) tbl[i] = 0u;
      __threadfence();
    }
    __syncthreads();
    const int* hist = P.hist + b * P.hist_stride;
    for (int t = tid; t < L; t += kThreads) {
      const int tok = hist[t];
      if (tok >= 0 && tok < V) {
        if (t >= g) atomicAdd(&tbl[tok], 1u);
        else atomicOr(&tbl[tok], kSeen);
      }
    }
    if (tid < e) {
      const int tok = P.draft[b * P.draft_stride + tid];
      if (tok >= 0 && tok < V) atomicAdd(&tbl[tok], 1u);
    }
    if constexpr (!LDS) __threadfence();
    __syncthreads();
  }

  // ---- steps 1 - 3, stored; the maximum of what is not a NaN
  const E* x_row = reinterpret_cast<const E*>(P.logits) + r * P.stride;
  float* o_row = P.out + r * P.out_stride;
  const float* b_row = P.bias ? P.bias + b * P.bias_stride : nullptr;
  const bool vin = (reinterpret_cast<uintptr_t>(x_row) & (4 * sizeof(E) - 1)) == 0;
  const bool vout = (reinterpret_cast<uintptr_t>(o_row) & 15) == 0;
  const bool vb = (reinterpret_cast<uintptr_t>(b_row) & 15) == 0;
  const int nch = (V + 3) >> 2;
  uint32_t best = 0u;                                               // below every key of a non-NaN float
  for (int c = tid; c < nch; c += kThreads) {
    const int i0 = c * 4, n = min(4, V - i0);
    float x[4], bi[4];
    uint32_t cn[4];
    load4<E>(x_row + i0, vin, n, x);
    if (b_row) load4<float>(b_row + i0, vb, n, bi);
#pragma unroll
    for (int q = 0; q < 4; ++q) cn[q] = 0u;
    if (ctx) {
      if constexpr (LDS) {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 v = reinterpret_cast<const u4*>(tbl)[c];
#pragma unroll
        for (int q = 0; q < 4; ++q) cn[q] = v[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < n) cn[q] = __hip_atomic_load(&tbl[i0 + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    float y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = x[q];
      if (!nan_bits(v)) {
        if (rep_on && cn[q] != 0u) {
          const uint32_t bits = __float_as_uint(v);
          const bool pos = bits != 0u && (bits >> 31) == 0u;
          v = pos ? v / theta : v * theta;
        }
        const uint32_t cnt = cn[q] & ~kSeen;
        if (cnt_on && cnt > 0u) {
          const float fc = fr * (float)cnt;
          v = v - fc;
          v = v - pr;
        }
        if (b_row) v = v + bi[q];
        if (q < n && !nan_bits(v)) best = max(best, okey(v));
      }
      y[q] = v;
    }
    if (vout && n == 4) {
      *reinterpret_cast<f32x4*>(o_row + i0) = f32x4{y[0], y[1], y[2], y[3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < n) o_row[i0 + q] = y[q];
    }
  }
  if (!floor_on) return;

  // ---- step 4: the row's maximum, then -inf over what this thread stored below m + gap
#pragma unroll
  for (int s = 32; s; s >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, s));
  if (lane == 0) redu[wid] = best;
  __syncthreads();
  best = max(max(redu[0], redu[1]), max(redu[2], redu[3]));
  if (best == 0u) return;                                           // V values, every one a NaN
  const float m = unkey(best);
  if (!finite_bits(m)) return;
  const float thr = m + gap;
  for (int c = tid; c < nch; c += kThreads) {
    const int i0 = c * 4, n = min(4, V - i0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < n) {
        const float v = o_row[i0 + q];
        if (!nan_bits(v) && !(v >= thr)) o_row[i0 + q] = -INFINITY;
      }
    }
  }
}

template <class E>
int launch_typed(const PenaltyParams& p, hipStream_t st) {
  const dim3 grid((unsigned)p.R), block(kThreads);
  if (p.V <= kLdsMaxV) {
    auto kern = penalize_rows_kernel<E, true>;
    // more than the default dynamic LDS limit.  The attribute belongs to the current device, so it is set
    // at every launch (a host call of no weight next to the launch), not once per process.
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxV * 4);
    if (attr != hipSuccess) return (int)attr;
    const size_t lds = (size_t)((p.V + 3) / 4) * 4 * sizeof(uint32_t);
    hipLaunchKernelGGL(kern, grid, block, lds, st, p);
  } else {
    hipLaunchKernelGGL((penalize_rows_kernel<E, false>), grid, block, 0, st, p);
  }
  return (int)hipGetLastError();
}

}  // namespace

size_t penalize_workspace_bytes(int64_t R, int64_t V) {
  return V > kLdsMaxV && R > 0 ? (size_t)R * (size_t)V * sizeof(uint32_t) : 0;
}

int launch_penalize(int dtype, const PenaltyParams& p, hipStream_t st) {
  if (p.R == 0) return 0;
  switch (dtype) {
    case 0: return launch_typed<__bf16>(p, st);
    case 1: return launch_typed<_Float16>(p, st);
    case 2: return launch_typed<float>(p, st);
    default: return -2;
  }
}

}  // namespace dta
