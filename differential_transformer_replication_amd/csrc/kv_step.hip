// kv_step.hip -- the row write of a ragged / paged decode or append step (dta_kv_step_rows), gfx950.
//
// Replaces, for the rows a step adds at per-sequence positions, the table gather, the two RoPE
// launches and the arange / where / gather / cat / index_put_ scatter of
// kv_cache._seq_attention_step + write_rows by one launch.  Row r of sequence b sits at
//   at = pos[b] + r,   real = r < counts[b] && at < t_cap
// and a thread owns 8 consecutive elements of one (row, head): a piece of Q_i, of K_i or of V.
//   Q_i  (with a table) rotated to table row min(at, t_cap - 1) into q_out, padding rows included
//   K_i  of a real row: rotated (with a table) and stored to the row's place in the cache
//   V    of a real row: copied there
// The place is row `at` of sequence b (contiguous cache), row at % P of page tbl[b][at / P]
// (paged pool; the page id is clamped into the pool before it forms an address), or, for an
// fp8 pool, the k_out temporary next to one slot per row for dta_kv_quant_rows.  A padding row
// stores no K and no V anywhere.  The rotation is rope_kernel's (elementwise.hip): the same
// fp32 products rounded in the same places (rotate8), so the bits are dta_rope's.
// Elementwise and tiny: 16-byte loads and stores, every offset 64-bit, no LDS, no atomics.
#include "../../include/diffattn.h"
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;

template <class E>
__device__ __forceinline__ void ld8(const E* p, float* f) {
  if constexpr (sizeof(E) == 2) {
    typedef E v8 __attribute__((ext_vector_type(8)));
    const v8 v = *reinterpret_cast<const v8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[j + 4] = b[j]; }
  }
}
// plain stores: the decode launch that follows reads these rows back
template <class E>
__device__ __forceinline__ void st8(E* p, const float* f) {
  if constexpr (sizeof(E) == 2) {
    typedef E v8 __attribute__((ext_vector_type(8)));
    v8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (E)f[j];
    *reinterpret_cast<v8*>(p) = v;
  } else {
    *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
  }
}

// 8 elements = 4 interleaved pairs at element d of a head row, table row t: rope_kernel's lines
__device__ __forceinline__ void rotate8(const float* freqs, int64_t t, int HS, int d, const float* x, float* o) {
  const float* f = freqs + (t * (HS / 2) + d / 2) * 2;
  const f32x4 f0 = *reinterpret_cast<const f32x4*>(f), f1 = *reinterpret_cast<const f32x4*>(f + 4);
  const float fr[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float cs = fr[2 * j], sn = fr[2 * j + 1];
    const float a = x[2 * j], bb = x[2 * j + 1];
    // (a + ib)(cos + i sin) = (a cs - bb sn) + i (a sn + bb cs).  Which product of each sum is rounded
    // before the fused multiply-add decides the last bit, and the compiler's choice for the plain
    // expressions is not rope_kernel's here (whose sn passes through a select): spelled out, the
    // roundings are rope_kernel's -- bb * sn, then a * sn.
    o[2 * j] = __builtin_fmaf(a, cs, -(bb * sn));
    o[2 * j + 1] = __builtin_fmaf(bb, cs, a * sn);
  }
}

struct StepDiv { FastDiv row, Tn, head, HS; uint32_t per_row, per_head, total, nq, nk; };

template <class E>
__global__ __launch_bounds__(kThreads) void kv_step_rows_kernel(KvStepParams p, StepDiv dv) {
  const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= dv.total) return;
  const uint32_t row = dv.row.div(idx), within = idx - row * dv.per_row;
  const uint32_t b = dv.Tn.div(row), r = row - b * p.Tn;
  // no device value forms an address unclamped: pos into [0, t_cap], the page id into the pool
  const int at = min(max(p.pos[b], 0), p.t_cap) + (int)r;
  const bool real = (int)r < p.cnt[b] && at < p.t_cap;
  const int shift = p.shift, in_page = at & ((1 << shift) - 1);
  int page = 0;
  if (p.kind != DTA_KV_STEP_CONTIGUOUS && real)
    page = min(max(p.tbl[(int64_t)b * p.max_pages + (at >> shift)], 0), p.n_pages - 1);
  if (p.kind == DTA_KV_STEP_SLOTS && within == 0)      // a padding row: its slot of the spare page
    p.slots[row] = ((real ? page : p.n_pages) << shift) + in_page;
  if (dv.per_head == 0) return;                        // slots alone (an fp8 pool without RoPE)
  // where a real row's K_i / V go: (sequence, row) of the cache, (page, row) of the pool, (b, r) of k_out
  int64_t d0 = b, d1 = r;
  if (p.kind == DTA_KV_STEP_CONTIGUOUS) d1 = at;
  else if (p.kind == DTA_KV_STEP_PAGED) { d0 = page; d1 = in_page; }

  const uint32_t h = dv.head.div(within), c = within - h * dv.per_head;
  float x[8], o[8];
  if (c < dv.nq + dv.nk) {
    const bool isq = c < dv.nq;
    if (!isq && !real) return;
    const uint32_t e = (isq ? c : c - dv.nq) * 8;
    const uint32_t i = dv.HS.div(e), d = e - i * p.HS;
    const T5& s = isq ? p.q : p.k;
    ld8<E>(reinterpret_cast<const E*>(s.p) + b * s.sb + (int64_t)r * s.st + h * s.sh + i * s.si + d, x);
    E* dst;
    if (isq) {
      dst = reinterpret_cast<E*>(p.qo.p) + b * p.qo.sb + (int64_t)r * p.qo.st + h * p.qo.sh + i * p.qo.si + d;
    } else {
      dst = reinterpret_cast<E*>(p.kd.p) + d0 * p.kd.sb + d1 * p.kd.st + h * p.kd.sh + i * p.kd.si + d;
    }
    if (p.freqs) {
      rotate8(p.freqs, min(at, p.t_cap - 1), p.HS, (int)d, x, o);
      st8<E>(dst, o);
    } else {
      st8<E>(dst, x);
    }
  } else {
    if (!real) return;
    const uint32_t e = (c - dv.nq - dv.nk) * 8;
    ld8<E>(reinterpret_cast<const E*>(p.v.p) + b * p.v.sb + (int64_t)r * p.v.st + h * p.v.sh + e, x);
    st8<E>(reinterpret_cast<E*>(p.vd.p) + d0 * p.vd.sb + d1 * p.vd.st + h * p.vd.sh + e, x);
  }
}

}  // namespace

int launch_kv_step(int dtype, const KvStepParams& p, hipStream_t st) {
  const int64_t rows = (int64_t)p.B * p.Tn;
  if (rows == 0) return 0;
  StepDiv dv;
  const bool slots = p.kind == DTA_KV_STEP_SLOTS;
  dv.nq = p.freqs ? (uint32_t)(p.N * p.HS / 8) : 0u;               // Q_i pieces: only a rotation moves them
  dv.nk = (p.freqs || !slots) ? (uint32_t)(p.N * p.HS / 8) : 0u;    // K_i: rotated, or copied into a cache
  const uint32_t nv = slots ? 0u : (uint32_t)(p.DV / 8);            // V: the quantising write reads it in place
  dv.per_head = dv.nq + dv.nk + nv;
  dv.per_row = dv.per_head ? (uint32_t)p.H * dv.per_head : 1u;
  const int64_t total = rows * dv.per_row;
  if (total >= (1ll << 31)) return -2;
  dv.total = (uint32_t)total;
  dv.row = FastDiv(dv.per_row);
  dv.Tn = FastDiv((uint32_t)p.Tn);
  dv.head = FastDiv(dv.per_head ? dv.per_head : 1u);
  dv.HS = FastDiv((uint32_t)p.HS);
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
  switch (dtype) {
    case 0: hipLaunchKernelGGL(kv_step_rows_kernel<__bf16>, grid, dim3(kThreads), 0, st, p, dv); break;
    case 1: hipLaunchKernelGGL(kv_step_rows_kernel<_Float16>, grid, dim3(kThreads), 0, st, p, dv); break;
    case 2: hipLaunchKernelGGL(kv_step_rows_kernel<float>, grid, dim3(kThreads), 0, st, p, dv); break;
    default: return -2;
  }
  return (int)hipGetLastError();
}

}  // namespace dta
