// kv_quant.hip -- the write side of the fp8 paged KV cache (dta_kv_quant_rows), gfx950.
//
// Replaces the index_put_ that scatters a step's new K_i / V rows into the page pool
// (kv_cache._paged_attention_step) when the pool holds OCP e4m3fn bytes: every vector x
// (a K_i head row of hs values, or a V head row of dv values) becomes
//   amax  = max|x|                      fp32, from the values as the activation dtype stores them
//   scale = amax / 448                  one fp32 per (row, head, K_i | V)
//   byte  = e4m3_rne(clamp(x / scale, -448, 448))      amax == 0: scale 0, bytes 0, no division
// The clamp is explicit: nothing relies on what v_cvt_pk_fp8_f32 does past the range.
// A lane owns 16 consecutive elements (hs, dv % 16 == 0, so a lane never straddles two
// vectors): 32 or 64 bytes in, one 16-byte store out.  The (N*hs + dv) / 16 lanes of one
// (row, head) sit in one wave (16, 32 or 64 lanes reserved for them), the amax of a vector
// is a shuffle walk over its lanes, and the vector's first lane stores the scale.
// slot = page * P + row comes from the device and is clamped into the pool (its spare
// page included) before it forms an address.
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;

template <class E>
__device__ __forceinline__ void ld16f(const E* p, float* f) {
  if constexpr (sizeof(E) == 2) {
    typedef E v8 __attribute__((ext_vector_type(8)));
    const v8 a = *reinterpret_cast<const v8*>(p), b = *reinterpret_cast<const v8*>(p + 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = (float)a[j]; f[j + 8] = (float)b[j]; }
  } else {
    const f32x4* q = reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 a = q[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * c + j] = a[j];
    }
  }
}

// LP: lanes reserved per (row, head), a power of two >= (N*HS + DV) / 16
template <class E, int LP>
__global__ __launch_bounds__(kThreads) void kv_quant_rows_kernel(KvQuantParams p) {
  const int item = blockIdx.x * (kThreads / LP) + threadIdx.x / LP;     // (row, head)
  const int l = threadIdx.x % LP;
  const int items = p.B * p.Tn * p.H;
  const int nk = p.N * p.HS;                      // K elements of one (row, head)
  const int used = (nk + p.DV) / 16;              // lanes that hold data
  const bool live = item < items && l < used;
  // this lane's vector: branch vi < N of K, or V (vi = N); its first lane and lane count
  const int e0 = l * 16;
  const bool isv = e0 >= nk;
  const int vi = isv ? p.N : e0 / p.HS;
  const int seg0 = isv ? nk / 16 : vi * (p.HS / 16);
  const int segn = (isv ? p.DV : p.HS) / 16;
  const int d0 = e0 - seg0 * 16;                  // offset inside the vector
  const int it = min(item, items - 1);
  const int h = it % p.H, r = it / p.H, t = r % p.Tn, b = r / p.Tn;

  float x[16];
  float am = 0.f;
  if (live) {
    const E* src = isv ? reinterpret_cast<const E*>(p.vsrc.p) + b * p.vsrc.sb + t * p.vsrc.st + h * p.vsrc.sh + d0
                       : reinterpret_cast<const E*>(p.ksrc.p) + b * p.ksrc.sb + t * p.ksrc.st + h * p.ksrc.sh +
                             vi * p.ksrc.si + d0;
    ld16f<E>(src, x);
#pragma unroll
    for (int u = 0; u < 16; ++u) am = fmaxf(am, fabsf(x[u]));
  }
  // amax over the vector's lanes (all lanes of the wave walk the longest vector: <= 16 steps)
  const int base = (threadIdx.x & 63) - l + seg0;
  const int steps = max(p.HS, p.DV) / 16;
  float amax = 0.f;
  for (int k = 0; k < steps; ++k) {
    const float o = __shfl(am, base + min(k, segn - 1), 64);
    amax = fmaxf(amax, o);
  }
  if (!live) return;

  const float scale = amax / 448.f;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (amax > 0.f) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) y[u] = fminf(fmaxf(x[4 * c + u] / scale, -448.f), 448.f);
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], pk, true);
      w[c] = (uint32_t)pk;
    }
  }
  const int slot = min(max(p.slot[r], 0), p.slots - 1);
  const int page = slot >> p.shift, row = slot & ((1 << p.shift) - 1);
  uint8_t* dst = isv ? reinterpret_cast<uint8_t*>(p.vdst.p) + page * p.vdst.sb + row * p.vdst.st + h * p.vdst.sh + d0
                     : reinterpret_cast<uint8_t*>(p.kdst.p) + page * p.kdst.sb + row * p.kdst.st + h * p.kdst.sh +
                           vi * p.kdst.si + d0;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
  if (d0 == 0) p.kvs[(int64_t)page * p.kvs_sb + ((int64_t)row * p.H + h) * (p.N + 1) + vi] = scale;
}

template <class E>
int quant_launch(const KvQuantParams& p, hipStream_t st) {
  const int used = (p.N * p.HS + p.DV) / 16;
  const int64_t items = (int64_t)p.B * p.Tn * p.H;
  if (used > 64 || items > INT32_MAX) return -2;
  const int lp = used <= 16 ? 16 : used <= 32 ? 32 : 64;
  const dim3 grid((unsigned)((items + kThreads / lp - 1) / (kThreads / lp)));
  switch (lp) {
    case 16: hipLaunchKernelGGL((kv_quant_rows_kernel<E, 16>), grid, dim3(kThreads), 0, st, p); break;
    case 32: hipLaunchKernelGGL((kv_quant_rows_kernel<E, 32>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((kv_quant_rows_kernel<E, 64>), grid, dim3(kThreads), 0, st, p); break;
  }
  return (int)hipGetLastError();
}

}  // namespace

int launch_kv_quant(int dtype, const KvQuantParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.Tn * p.H == 0) return 0;
  switch (dtype) {
    case 0: return quant_launch<__bf16>(p, st);
    case 1: return quant_launch<_Float16>(p, st);
    case 2: return quant_launch<float>(p, st);
  }
  return -2;
}

}  // namespace dta
