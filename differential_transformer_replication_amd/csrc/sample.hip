// sample.hip -- seeded temperature / top-k / top-p sampling of logits rows (dta_sample_rows), gfx950.
//
// One 256-thread workgroup per row, one token (and optionally its log-probability) per row.  The
// definition is include/diffattn.h's ("Sampling"); what this file adds is the shape of the work.
//
//   * Element i of a row belongs to chunk c = i / 8, and chunk c to thread c % 256 in round c / 256,
//     whichever way it is loaded (16-byte loads when the row's first byte is 16-byte aligned, element
//     loads otherwise) and wherever it is read from (a row of V <= kStageMax is staged once into LDS
//     as fp32, padded with -inf to a multiple of 8; a longer one is re-read from L2 by every pass).
//     So no float depends on alignment, on the row's index or on R.
//   * Comparisons run on the order-preserving uint32 image of the fp32 logit (-0 is read as +0),
//     shifted right by the bits a 16-bit dtype leaves constant (bf16: 16, f16: 13).
//   * A masked sum S(lim) = sum of w_i over key_i >= lim: per thread, the 8 weights of a chunk are
//     summed as a 3-level tree and the chunk sums are added in round order; 64 lanes are combined by
//     an xor butterfly (6 levels), the 4 waves as ((s0 + s1) + s2) + s3.  Masked-out terms are +0, and
//     round-to-nearest addition is monotone, so S is monotone in the mask: the bisections below are exact.
//   * top-k: the k-th largest key is the least t with #{key > t} < k -- one integer count per key bit.
//     top-p: the least t with S(max(kth, t + 1)) < p * S(kth), bisected over the bits in which the
//     k-th and the largest key differ.  (A radix select would take fewer passes for top-k; the
//     count passes share the sum's loop and are cheap next to it.)
//   * The draw walks the row in tiles of 2048 elements: chunk-local inclusive prefixes, a shuffle
//     scan over the lanes, the waves' totals in order, the carry of the earlier tiles; the lowest kept
//     index whose prefix exceeds u * Z wins (an integer min).  Longest add chain, over the sum and the
//     scan: D(V) = ceil(V / 2048) + 20.
// No floating-point atomics, no LDS atomics, no generator state: u is Philox4x32-10 of (seed, stream,
// offset), computed by every thread.  -fno-honor-nans is in force for this library, so every NaN test
// here is on the bits.
#include "../../include/diffattn.h"
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;
constexpr int kStageMax = 15360;            // 60 KiB of fp32: the static arrays fit beside it in 64 KiB
constexpr uint32_t kNone = 0xffffffffu;

template <class E> struct KeyLow { static constexpr int v = 0; };
template <> struct KeyLow<__bf16> { static constexpr int v = 16; };
template <> struct KeyLow<_Float16> { static constexpr int v = 13; };

__device__ __forceinline__ uint32_t okey(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ bool nan_bits(float x) { return (__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u; }
// -0 -> +0, so that the key order is the order of the values
__device__ __forceinline__ float canon(float x) { return __float_as_uint(x) == 0x80000000u ? 0.f : x; }

// chunk c of a row in global memory; elements past V read as -inf
template <class E>
__device__ __forceinline__ void gload8(const E* g, int c, int V, bool vec, float* x) {
  const int i0 = c * 8;
  if (vec && i0 + 8 <= V) {
    if constexpr (sizeof(E) == 2) {
      typedef E v8 __attribute__((ext_vector_type(8)));
      const v8 v = *reinterpret_cast<const v8*>(g + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = canon((float)v[j]);
    } else {
      const f32x4 a = *reinterpret_cast<const f32x4*>(g + i0), b = *reinterpret_cast<const f32x4*>(g + i0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { x[j] = canon(a[j]); x[j + 4] = canon(b[j]); }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = i0 + j < V ? canon((float)g[i0 + j]) : -INFINITY;
  }
}

__device__ __forceinline__ uint32_t philox_u32(uint64_t seed, uint64_t off, uint64_t strm) {
  uint32_t c0 = (uint32_t)off, c1 = (uint32_t)(off >> 32), c2 = (uint32_t)strm, c3 = (uint32_t)(strm >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// the workgroup's exchange: two sets of four slots, used alternately, so one barrier per reduction
struct Xchg {
  float* f; uint32_t* u; int par, lane, wid;
  __device__ __forceinline__ float sum(float v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    float* s = f + par * 4;
    if (lane == 0) s[wid] = v;
    __syncthreads();
    par ^= 1;
    return ((s[0] + s[1]) + s[2]) + s[3];
  }
  template <bool MIN>
  __device__ __forceinline__ uint32_t fold(uint32_t v) {           // sum, or min
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = MIN ? min(v, o) : v + o; }
    uint32_t* s = u + par * 4;
    if (lane == 0) s[wid] = v;
    __syncthreads();
    par ^= 1;
    return MIN ? min(min(s[0], s[1]), min(s[2], s[3])) : s[0] + s[1] + s[2] + s[3];
  }
};

// least t in [prefix, prefix | (2 << b0) - 1] with q(t) true; q is monotone and true at the range's end
template <class Q>
__device__ __forceinline__ uint32_t bisect(int b0, uint32_t prefix, Q q) {
  uint32_t ans = prefix;
  for (int b = b0; b >= 0; --b)
    if (!q(ans | ((1u << b) - 1u))) ans |= 1u << b;               // bit b of the trial is 0: trial + 1 cannot wrap
  return ans;
}

template <class E, bool ST>
__global__ __launch_bounds__(kThreads) void sample_rows_kernel(SampleParams P) {
  extern __shared__ float sx[];
  __shared__ float redf[8];
  __shared__ uint32_t redu[8];
  __shared__ unsigned long long red64[4];
  constexpr int LOW = KeyLow<E>::v, KB = 32 - LOW;
  const int tid = threadIdx.x;
  Xchg xc{redf, redu, 0, tid & 63, tid >> 6};
  const int64_t r = blockIdx.x;
  const E* g = reinterpret_cast<const E*>(P.logits) + r * P.stride;
  const int V = P.V, nch = (V + 7) >> 3;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;

  auto load = [&](int c, float* x) {
    if constexpr (ST) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(sx + c * 8), b = *reinterpret_cast<const f32x4*>(sx + c * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { x[j] = a[j]; x[j + 4] = b[j]; }
    } else {
      gload8<E>(g, c, V, vec, x);
    }
  };

  // ---- the row's maximum, its lowest index, and whether the row is degenerate
  unsigned long long best = 0;
  int bad = 0;
  for (int c = tid; c < nch; c += kThreads) {
    float x[8];
    gload8<E>(g, c, V, vec, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = __float_as_uint(x[j]);
      bad |= ((b & 0x7fffffffu) > 0x7f800000u) || b == 0x7f800000u;
      const unsigned long long pk = ((unsigned long long)okey(x[j]) << 32) | (kNone - (uint32_t)(c * 8 + j));
      best = pk > best ? pk : best;
    }
    if constexpr (ST) {
      *reinterpret_cast<f32x4*>(sx + c * 8) = f32x4{x[0], x[1], x[2], x[3]};
      *reinterpret_cast<f32x4*>(sx + c * 8 + 4) = f32x4{x[4], x[5], x[6], x[7]};
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), d), lo = __shfl_xor((uint32_t)best, d);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o > best ? o : best;
  }
  if (xc.lane == 0) red64[xc.wid] = best;
  bad = __syncthreads_or(bad);                                     // also: the staged row is visible
#pragma unroll
  for (int w = 0; w < 4; ++w) best = red64[w] > best ? red64[w] : best;
  const uint32_t mkey = (uint32_t)(best >> 32), amax = kNone - (uint32_t)best;
  const float m = unkey(mkey);
  float* lp = P.lp ? P.lp + r : nullptr;
  if (bad || mkey == 0x007fffffu) {                                // NaN, +inf, or every logit -inf
    if (tid == 0) {
      P.tok[r] = -1;
      if (lp) *reinterpret_cast<uint32_t*>(lp) = 0x7fc00000u;
    }
    return;
  }

  float T = P.Tdev ? P.Tdev[r] : P.T;
  const bool greedy = nan_bits(T) || T <= 0.f;
  if (greedy) T = 1.f;
  const bool unit = T == 1.f;
  auto weight = [&](float x) { const float d = x - m; return expf(unit ? d : d / T); };
  // S(lim): the sum of the weights whose key is >= lim, in the fixed shape of the header comment
  auto wsum = [&](uint32_t lim) {
    float acc = 0.f;
    for (int c = tid; c < nch; c += kThreads) {
      float x[8], a[8];
      load(c, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (okey(x[j]) >> LOW) >= lim ? weight(x[j]) : 0.f;
      acc += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    return xc.sum(acc);
  };
  auto count = [&](uint32_t lim) {
    uint32_t n = 0;
    for (int c = tid; c < nch; c += kThreads) {
      float x[8];
      load(c, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) n += (okey(x[j]) >> LOW) >= lim;
    }
    return xc.fold<false>(n);
  };

  if (greedy) {
    if (lp) {                                                      // every thread takes part in the sum
      const float S = wsum(0u);
      if (tid == 0) *lp = -logf(S);
    }
    if (tid == 0) P.tok[r] = (int64_t)amax;
    return;
  }

  const int k = P.kdev ? P.kdev[r] : P.k;
  const float p = P.pdev ? P.pdev[r] : P.p;
  const uint32_t hk = mkey >> LOW;
  uint32_t lo = 0u;
  if (k > 0 && k < V)
    lo = k == 1 ? hk : bisect(KB - 1, 0u, [&](uint32_t t) { return count(t + 1u) < (uint32_t)k; });
  float Z = wsum(lo);
  if (!nan_bits(p) && p > 0.f && p < 1.f && lo != hk) {
    const float thr = p * Z;
    const int b0 = 31 - __clz(lo ^ hk);
    const uint32_t t = bisect(b0, hk & ~((2u << b0) - 1u), [&](uint32_t t) { return wsum(max(lo, t + 1u)) < thr; });
    lo = max(lo, t);
    Z = wsum(lo);
  }

  // ---- the draw
  const uint64_t strm = P.strm ? (uint64_t)P.strm[r] : (uint64_t)r;
  const uint64_t off = P.off ? (uint64_t)P.off[r] : 0ull;
  const float u = (float)(philox_u32(P.seed, off, strm) >> 8) * 0x1p-24f;
  const float target = u * Z;
  float carry = 0.f;
  uint32_t tok = kNone;
  for (int c0 = 0; c0 < nch; c0 += kThreads) {
    const int c = c0 + tid;
    float pre[8];
    uint32_t kept = 0;
    if (c < nch) {
      float x[8];
      load(c, x);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = (okey(x[j]) >> LOW) >= lo && c * 8 + j < V;
        kept |= (uint32_t)in << j;
        s += in ? weight(x[j]) : 0.f;
        pre[j] = s;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) pre[j] = 0.f;
    }
    float incl = pre[7];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o = __shfl_up(incl, d);
      if (xc.lane >= d) incl += o;
    }
    float excl = __shfl_up(incl, 1);
    if (xc.lane == 0) excl = 0.f;
    float* s4 = xc.f + xc.par * 4;
    if (xc.lane == 63) s4[xc.wid] = incl;
    __syncthreads();
    xc.par ^= 1;
    float woff = 0.f;
    for (int w = 0; w < xc.wid; ++w) woff += s4[w];
    const float base = (carry + woff) + excl;
    carry += ((s4[0] + s4[1]) + s4[2]) + s4[3];
    uint32_t cand = kNone;
#pragma unroll
    for (int j = 7; j >= 0; --j)
      if (((kept >> j) & 1u) && base + pre[j] > target) cand = (uint32_t)(c * 8 + j);
    tok = xc.fold<true>(cand);
    if (tok != kNone) break;
  }
  if (tok == kNone) {                                              // rounding left none: the last kept index
    uint32_t last = 0u;                                            // as min over kNone - 1 - index
    uint32_t inv = kNone;
    for (int c = tid; c < nch; c += kThreads) {
      float x[8];
      load(c, x);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if ((okey(x[j]) >> LOW) >= lo && c * 8 + j < V) inv = min(inv, kNone - 1u - (uint32_t)(c * 8 + j));
    }
    inv = xc.fold<true>(inv);
    last = kNone - 1u - inv;
    tok = inv == kNone ? amax : last;
  }
  if (tid == 0) {
    P.tok[r] = (int64_t)tok;
    if (lp) {
      const float xt = ST ? sx[tok] : canon((float)g[tok]);
      const float d = xt - m;
      *lp = (unit ? d : d / T) - logf(Z);
    }
  }
}

template <class E>
int launch_typed(const SampleParams& p, hipStream_t st) {
  const dim3 grid((unsigned)p.R), block(kThreads);
  if (p.V <= kStageMax) {
    const size_t lds = (size_t)((p.V + 7) / 8) * 8 * sizeof(float);
    hipLaunchKernelGGL((sample_rows_kernel<E, true>), grid, block, lds, st, p);
  } else {
    hipLaunchKernelGGL((sample_rows_kernel<E, false>), grid, block, 0, st, p);
  }
  return (int)hipGetLastError();
}

}  // namespace

int launch_sample(int dtype, const SampleParams& p, hipStream_t st) {
  if (p.R == 0) return 0;
  switch (dtype) {
    case 0: return launch_typed<__bf16>(p, st);
    case 1: return launch_typed<_Float16>(p, st);
    case 2: return launch_typed<float>(p, st);
    default: return -2;
  }
}

}  // namespace dta
