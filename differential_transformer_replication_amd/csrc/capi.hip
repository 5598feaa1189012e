// capi.hip -- the extern "C" boundary of libdiffattn.so (include/diffattn.h).
// Validates every argument, then enqueues kernels on the caller's stream.
// Nothing here allocates, synchronises or keeps state.
#include "../../include/diffattn.h"
#include "dta_internal.h"

namespace dta {
int launch_attn_fwd_bf16(const FwdParams&, hipStream_t);
int launch_attn_fwd_f16(const FwdParams&, hipStream_t);
int launch_attn_fwd_f32(const FwdParams&, hipStream_t);
int launch_attn_dq_bf16(const BwdParams&, hipStream_t);
int launch_attn_dq_f16(const BwdParams&, hipStream_t);
int launch_attn_dq_f32(const BwdParams&, hipStream_t);
int launch_attn_dkdv_bf16(const BwdParams&, hipStream_t);
int launch_attn_dkdv_f16(const BwdParams&, hipStream_t);
int launch_attn_dkdv_f32(const BwdParams&, hipStream_t);
int launch_attn_fwd_bf16_drop(const FwdParams&, hipStream_t);
int launch_attn_fwd_f16_drop(const FwdParams&, hipStream_t);
int launch_attn_fwd_f32_drop(const FwdParams&, hipStream_t);
int launch_attn_dq_bf16_drop(const BwdParams&, hipStream_t);
int launch_attn_dq_f16_drop(const BwdParams&, hipStream_t);
int launch_attn_dq_f32_drop(const BwdParams&, hipStream_t);
int launch_attn_dkdv_bf16_drop(const BwdParams&, hipStream_t);
int launch_attn_dkdv_f16_drop(const BwdParams&, hipStream_t);
int launch_attn_dkdv_f32_drop(const BwdParams&, hipStream_t);
bool attn_native_bf16(int, int, int);
bool attn_native_f16(int, int, int);
bool attn_native_f32(int, int, int);

int launch_attn_fwd(int dtype, const FwdParams& p, hipStream_t st) {
  if (p.drop_thr) switch (dtype) {
    case DTA_BF16: return launch_attn_fwd_bf16_drop(p, st);
    case DTA_F16: return launch_attn_fwd_f16_drop(p, st);
    case DTA_F32: return launch_attn_fwd_f32_drop(p, st);
  }
  switch (dtype) {
    case DTA_BF16: return launch_attn_fwd_bf16(p, st);
    case DTA_F16: return launch_attn_fwd_f16(p, st);
    case DTA_F32: return launch_attn_fwd_f32(p, st);
  }
  return -2;
}
int launch_attn_dq(int dtype, const BwdParams& p, hipStream_t st) {
  if (p.drop_thr) switch (dtype) {
    case DTA_BF16: return launch_attn_dq_bf16_drop(p, st);
    case DTA_F16: return launch_attn_dq_f16_drop(p, st);
    case DTA_F32: return launch_attn_dq_f32_drop(p, st);
  }
  switch (dtype) {
    case DTA_BF16: return launch_attn_dq_bf16(p, st);
    case DTA_F16: return launch_attn_dq_f16(p, st);
    case DTA_F32: return launch_attn_dq_f32(p, st);
  }
  return -2;
}
int launch_attn_dkdv(int dtype, const BwdParams& p, hipStream_t st) {
  if (p.drop_thr) switch (dtype) {
    case DTA_BF16: return launch_attn_dkdv_bf16_drop(p, st);
    case DTA_F16: return launch_attn_dkdv_f16_drop(p, st);
    case DTA_F32: return launch_attn_dkdv_f32_drop(p, st);
  }
  switch (dtype) {
    case DTA_BF16: return launch_attn_dkdv_bf16(p, st);
    case DTA_F16: return launch_attn_dkdv_f16(p, st);
    case DTA_F32: return launch_attn_dkdv_f32(p, st);
  }
  return -2;
}
bool attn_native(int dtype, int hs, int n, int dv) {
  // dv = 2 hs (differential models) or, for standard attention (N = 1), dv = hs
  if (dv != 2 * hs && !(n == 1 && dv == hs)) return false;
  switch (dtype) {
    case DTA_BF16: return attn_native_bf16(hs, n, dv);
    case DTA_F16: return attn_native_f16(hs, n, dv);
    case DTA_F32: return attn_native_f32(hs, n, dv);
  }
  return false;
}
// Every branch count runs: natively, or -- where no N-branch plan is built (N >= 5, fp32
// N = 3 / 4 at head sizes 96 / 128) -- as branch groups that each have one, on top of the
// single-branch plan (the forward then runs branch-split, the backward group by group).
bool attn_supported(int dtype, int hs, int n, int dv) {
  if (n < 1) return false;
  return attn_native(dtype, hs, n, dv) || (n >= 2 && dv == 2 * hs && attn_native(dtype, hs, 1, dv));
}
// size of the next branch group of the backward: the largest native branch count <= cap
int branch_group(int dtype, int hs, int left, int dv, int cap) {
  for (int g = left < cap ? left : cap; g > 1; --g)
    if (attn_native(dtype, hs, g, dv)) return g;
  return 1;
}
// largest backward branch group per stage (16-bit; fp32 keeps 4).  The 3- / 4-branch
// backward plans at head size >= 64 have no room for the paired two-waves-per-SIMD layout
// (Q rows, K/V tiles and accumulators of 3-4 branches overflow 80 KB of LDS and 256 VGPRs)
// and run one wave per SIMD with spills; groups of <= 2 branches recompute dP = dO V^T once
// per group but run the paired plans.  Measured per kernel (profiles/r04_bwd_groups.json,
// bf16, native -> groups of two): dK/dV hs 64 N = 3 0.464 -> 0.44 ms, hs 96 N = 4 11.6 ->
// 3.4 ms, hs 128 N = 4 8.4 -> 2.9 ms; dQ hs 128 N = 4 4.0 -> 2.0 ms, but dQ at hs 64 / 96
// N = 3 0.40 -> 0.45 / 1.69 -> 1.84 ms and hs 96 N = 4 2.27 -> 2.35 ms, so dQ groups at
// head size 128, and at 64 for N >= 4 (0.487 either way: no re-base needed).  Head size 32
// keeps the native plans for both.  Where the two groupings differ, the delta rows take the
// dK/dV grouping's encoding: written so by attn_dq when one dQ launch holds every branch
// (round 6, BwdParams::kstarts, profiles/r06t_ab_dq_kstarts.json), else re-based after the
// dQ launches (delta_rebase_kernel, ~3-7 us, profiles/r04_bwd_rebase.json).
int bwd_group_cap(int dtype, int hs, int n, bool dkdv) {
  if (dtype == DTA_F32) return 4;
  if (hs >= 192) return 1;            // head size 256: the single-branch plans (the N = 2 ones spill)
  if (dkdv) return hs >= 64 ? 2 : 4;
  return (hs >= 128 || (hs >= 64 && hs < 96 && n >= 4)) ? 2 : 4;
}
// group starts of the backward of an N-branch problem as a bit mask (bit i: a group
// starts at branch i)
uint64_t group_starts(int dtype, int hs, int n, int dv, int cap) {
  uint64_t m = 0;
  for (int g0 = 0, ng; g0 < n; g0 += ng) {
    ng = branch_group(dtype, hs, n - g0, dv, cap);
    m |= 1ull << g0;
  }
  return m;
}
}  // namespace dta

using namespace dta;

namespace {

constexpr float kLog2e = 1.4426950408889634f;

int esize(int dtype) { return dtype == DTA_F32 ? 4 : 2; }

// attention dropout probability -> (keep threshold on a 32-bit hash, 1/(1-p)); p in [0, 1)
bool drop_params(float p, uint64_t seed, uint32_t& thr, float& scale, uint32_t& lo, uint32_t& hi) {
  if (!(p >= 0.f && p < 1.f)) return false;
  const double t = (double)p * 4294967296.0;
  thr = p > 0.f ? (uint32_t)(t < 1.0 ? 1.0 : (t > 4294967295.0 ? 4294967295.0 : t)) : 0u;
  scale = p > 0.f ? (float)(1.0 / (1.0 - (double)p)) : 1.f;
  lo = (uint32_t)seed;
  hi = (uint32_t)(seed >> 32);
  return true;
}

// element alignment every pointer/stride must have: one 16-byte vector
int vec_elems(int dtype) { return 16 / esize(dtype); }

bool aligned_ptr(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

bool ok_tensor(const dta_tensor& t, int dtype, bool with_i) {
  const int64_t v = vec_elems(dtype);
  if (!aligned_ptr(t.ptr)) return false;
  if (t.sb % v || t.st % v || t.sh % v) return false;
  if (with_i && t.si % v) return false;
  return t.sb >= 0 && t.st >= 0 && t.sh >= 0 && t.si >= 0;
}

T5 t5(const dta_tensor& t) { return T5{t.ptr, t.sb, t.st, t.sh, t.si}; }

// obr (the per-branch O_i): fp32 (obr_dtype 0 or DTA_F32), or fp16 with 16-bit activations
bool ok_obr(const dta_tensor& t, int obr_dtype, int dtype) {
  if (obr_dtype == DTA_F16) return dtype != DTA_F32 && ok_tensor(t, DTA_F16, true);
  return (obr_dtype == 0 || obr_dtype == DTA_F32) && ok_tensor(t, DTA_F32, true);
}

int status(int e) {
  if (e == 0) return DTA_OK;
  if (e == -2) return DTA_ERR_UNSUPPORTED;
  return DTA_ERR_LAUNCH;
}

bool ok_dims(int dtype, int B, int T, int H, int N, int hs, int dv) {
  if (dtype < DTA_BF16 || dtype > DTA_F32) return false;
  return B >= 0 && T >= 0 && H > 0 && N > 0 && hs > 0 && dv > 0;
}

}  // namespace

#ifndef DTA_STAMPS
#define DTA_STAMPS 0
#endif
#if DTA_STAMPS
// diagnostic builds only: one device buffer for the kernels' per-wave stamp sums
static unsigned long long* stamp_buf() {
  static unsigned long long* b = [] {
    void* p = nullptr;
    if (hipMalloc(&p, 64 << 20) || hipMemset(p, 0, 64 << 20)) p = nullptr;
    return (unsigned long long*)p;
  }();
  return b;
}
#else
static unsigned long long* stamp_buf() { return nullptr; }
#endif

extern "C" {

#if DTA_STAMPS
// copy the stamp buffer to the host (diagnostic builds only; not in include/diffattn.h)
int dta_debug_stamps(void* dst, size_t bytes) {
  if (!stamp_buf() || bytes > (64u << 20)) return DTA_ERR_INVALID;
  return hipMemcpy(dst, stamp_buf(), bytes, hipMemcpyDeviceToHost) ? DTA_ERR_LAUNCH : DTA_OK;
}
#endif

int dta_abi_version(void) { return DTA_ABI_VERSION; }

const char* dta_error_string(int code) {
  switch (code) {
    case DTA_OK: return "ok";
    case DTA_ERR_INVALID: return "invalid argument (shape, null/misaligned pointer or stride)";
    case DTA_ERR_UNSUPPORTED: return "unsupported configuration (head_size/n_terms/dtype not built for gfx950)";
    case DTA_ERR_LAUNCH: return "HIP launch failed";
    case DTA_ERR_DROPOUT: return "attention dropout p must lie in [0, 1)";
  }
  return "unknown error";
}

int dta_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv) {
  return attn_supported(dtype, head_size, n_terms, dv) ? 1 : 0;
}

int dta_attn_fwd(const dta_attn_fwd_args* a, void* stream) {
  if (!a) return DTA_ERR_INVALID;
  if (!ok_dims(a->dtype, a->B, a->T, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  FwdParams p{};
  if (!drop_params(a->dropout_p, a->dropout_seed, p.drop_thr, p.drop_scale, p.drop_seed_lo, p.drop_seed_hi))
    return DTA_ERR_DROPOUT;
  if (!attn_supported(a->dtype, a->head_size, a->n_terms, a->dv)) return DTA_ERR_UNSUPPORTED;
  if ((int64_t)a->B * a->T == 0) return DTA_OK;
  if (!ok_tensor(a->q, a->dtype, true) || !ok_tensor(a->k, a->dtype, true) || !ok_tensor(a->v, a->dtype, false) ||
      !ok_tensor(a->o, a->dtype, false) || !ok_obr(a->obr, a->obr_dtype, a->dtype) || !a->lse || !a->coef)
    return DTA_ERR_INVALID;
  p.ob16 = a->obr_dtype == DTA_F16;
  p.q = t5(a->q); p.k = t5(a->k); p.v = t5(a->v); p.o = t5(a->o); p.obr = t5(a->obr);
  p.lse = a->lse; p.coef = a->coef;
  p.B = a->B; p.T = a->T; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.sl2 = a->scale * kLog2e;
  p.cst = a->n_terms;
  if (a->rope_freqs) {
    if (a->head_size % 2 || ((uintptr_t)a->rope_freqs & 15) || !ok_tensor(a->q_rot, a->dtype, true)) return DTA_ERR_INVALID;
    p.rope = a->rope_freqs;
    p.qrot = t5(a->q_rot);
  }
  p.stamps = stamp_buf();
  return status(launch_attn_fwd(a->dtype, p, (hipStream_t)stream));
}

// dK/dV launches (branch groups) a backward of this shape runs at the default caps: more than
// one means dV is summed across groups (in dv_f32 when given)
int dta_attn_bwd_dkdv_groups(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t group_max_dkdv) {
  // a negative cap is invalid here as in dta_attn_bwd
  if (!attn_supported(dtype, head_size, n_terms, dv) || group_max_dkdv < 0) return 0;
  const int cap = group_max_dkdv > 0 ? group_max_dkdv : bwd_group_cap(dtype, head_size, n_terms, true);
  int n = 0;
  for (int g0 = 0, ng; g0 < n_terms; g0 += ng, ++n) ng = branch_group(dtype, head_size, n_terms - g0, dv, cap);
  return n;
}

size_t dta_attn_bwd_dcoef_partial_bytes(int32_t B, int32_t T, int32_t H, int32_t n_terms) {
  return (size_t)H * n_terms * B * ((T + 31) / 32) * 4;
}

size_t dta_attn_bwd_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t n_terms, int32_t head_size) {
  const size_t delta = (size_t)n_terms * B * H * T * 4;
  const size_t dq = (size_t)B * T * H * n_terms * head_size * 4;
  return delta + dq;
}

int dta_attn_bwd(const dta_attn_bwd_args* a, void* stream) {
  if (!a) return DTA_ERR_INVALID;
  if (!ok_dims(a->dtype, a->B, a->T, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  BwdParams p{};
  if (!drop_params(a->dropout_p, a->dropout_seed, p.drop_thr, p.drop_scale, p.drop_seed_lo, p.drop_seed_hi))
    return DTA_ERR_DROPOUT;
  if (!attn_supported(a->dtype, a->head_size, a->n_terms, a->dv)) return DTA_ERR_UNSUPPORTED;
  if (!a->dcoef) return DTA_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int stages = a->stages ? a->stages : (DTA_BWD_PRE | DTA_BWD_DQ | DTA_BWD_DKDV);
  // (with dcoef_partial the DQ stage's ordered reduce overwrites every dcoef entry: nothing to zero)
  const bool empty = (int64_t)a->B * a->T == 0;
  // no rows: the DQ stage launches nothing, so neither its ordered reduce nor its atomics reach
  // dcoef; the sum over no rows is zero, written here (a DKDV-only call leaves dcoef alone)
  if (((stages & DTA_BWD_PRE) && !a->dcoef_partial) || (empty && (stages & DTA_BWD_DQ))) {
    if (hipMemsetAsync(a->dcoef, 0, sizeof(float) * a->H * a->n_terms, st)) return DTA_ERR_LAUNCH;
  }
  if (empty) return DTA_OK;
  if (!ok_tensor(a->q, a->dtype, true) || !ok_tensor(a->k, a->dtype, true) || !ok_tensor(a->v, a->dtype, false) ||
      !ok_obr(a->obr, a->obr_dtype, a->dtype) || !ok_tensor(a->dout, a->dtype, false) ||
      !ok_tensor(a->dk, a->dtype, true) || !ok_tensor(a->dv_out, a->dtype, false) ||
      !a->lse || !a->coef || !a->delta)
    return DTA_ERR_INVALID;
  if (a->dq.ptr ? !ok_tensor(a->dq, a->dtype, true) : !aligned_ptr(a->dq_f32)) return DTA_ERR_INVALID;
  p.q = t5(a->q); p.k = t5(a->k); p.v = t5(a->v); p.obr = t5(a->obr); p.dout = t5(a->dout);
  p.ob16 = a->obr_dtype == DTA_F16;
  p.dq = t5(a->dq); p.dk = t5(a->dk); p.dv = t5(a->dv_out);
  p.lse = a->lse; p.delta = a->delta; p.coef = a->coef; p.dcoef = a->dcoef;
  p.dq32 = a->dq.ptr ? nullptr : a->dq_f32;
  if (a->rope_freqs && (a->head_size % 4 || reinterpret_cast<uintptr_t>(a->rope_freqs) % 16)) return DTA_ERR_INVALID;
  p.rope = a->rope_freqs;
  if (a->dcoef_partial && !aligned_ptr(a->dcoef_partial)) return DTA_ERR_INVALID;
  if (a->dv_f32 && !aligned_ptr(a->dv_f32)) return DTA_ERR_INVALID;
  if (a->lse_c && !aligned_ptr(a->lse_c)) return DTA_ERR_INVALID;
  // |c_i| folded into the key-major kernel's probabilities: 16-bit plans without dropout
  p.lsec = (a->lse_c && a->dtype != DTA_F32 && !p.drop_thr) ? a->lse_c : nullptr;
  p.dcoef_part = a->dcoef_partial;
  p.B = a->B; p.T = a->T; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.scale = a->scale; p.sl2 = a->scale * kLog2e;
  p.cst = a->n_terms; p.br0 = 0; p.dv_acc = 0;
  p.stamps = stamp_buf();
  // branch groups [g0, g0 + ng): a native N runs as one group; otherwise each group's
  // branch-indexed operands are offset to its first branch (coef / dcoef rows keep the
  // stride cst = N), so the kernels see an ng-branch problem
  const int es = esize(a->dtype);
  const int64_t rowvec = (int64_t)p.B * p.H * p.T, nblk = (p.T + 31) / 32;
  auto group = [&](int g0, int ng) {
    BwdParams q = p;
    auto off = [&](T5& t) { t.p = (char*)t.p + (int64_t)g0 * t.si * es; };
    off(q.q); off(q.k); off(q.dk);
    q.obr.p = (char*)q.obr.p + (int64_t)g0 * q.obr.si * (p.ob16 ? 2 : 4);
    if (q.dq.p) off(q.dq);
    if (q.dq32) q.dq32 += (int64_t)g0 * p.HS;
    q.lse += g0 * rowvec; q.delta += g0 * rowvec; q.coef += g0; q.dcoef += g0;
    if (q.lsec) q.lsec += g0 * rowvec;
    if (q.dcoef_part) q.dcoef_part += g0 * (int64_t)p.B * nblk;
    q.N = ng; q.br0 = g0; q.dv_acc = g0 > 0; q.dv_last = g0 + ng == p.N;
    return q;
  };
  int e = 0;
  // the dK/dV grouping must see delta rows encoded for its own groups (see bwd_group_cap)
  if (a->group_max_dq < 0 || a->group_max_dkdv < 0) return DTA_ERR_INVALID;
  const int kcap = a->group_max_dkdv ? a->group_max_dkdv : bwd_group_cap(a->dtype, p.HS, p.N, true);
  int qcap = a->group_max_dq ? a->group_max_dq : bwd_group_cap(a->dtype, p.HS, p.N, false);
  // beyond 64 branches the group-start masks do not fit: both stages take the dK/dV grouping
  if (p.N > 64) qcap = kcap;
  // with dropout the delta rows hold delta_i itself (no group encoding): nothing to re-base
  const bool rebase = qcap != kcap && !p.drop_thr;
  const uint64_t qstarts = rebase ? group_starts(a->dtype, p.HS, p.N, p.DV, qcap) : 0;
  const uint64_t kstarts = rebase ? group_starts(a->dtype, p.HS, p.N, p.DV, kcap) : 0;
  if (stages & DTA_BWD_DQ) {
    // one dQ launch over every branch writes the delta rows straight in the dK/dV encoding
    const bool direct = qstarts != kstarts && branch_group(a->dtype, p.HS, p.N, p.DV, qcap) == p.N;
    for (int g0 = 0, ng; g0 < p.N; g0 += ng) {
      ng = branch_group(a->dtype, p.HS, p.N - g0, p.DV, qcap);
      BwdParams q = group(g0, ng);
      q.kstarts = direct ? kstarts : 0;
      if ((e = launch_attn_dq(a->dtype, q, st))) return status(e);
    }
    if (p.dcoef_part &&
        (e = launch_dcoef_reduce(p.dcoef_part, p.dcoef, p.H, p.N, (int64_t)p.B * nblk, st)))
      return status(e);
    if (!direct && qstarts != kstarts && (e = launch_delta_rebase(p.delta, rowvec, p.N, qstarts, kstarts, st)))
      return status(e);
  }
  if (stages & DTA_BWD_DKDV) {
    // more than one dK/dV group: dV is summed in the fp32 workspace when the caller gave one
    const bool multi = branch_group(a->dtype, p.HS, p.N, p.DV, kcap) < p.N;
    for (int g0 = 0, ng; g0 < p.N; g0 += ng) {
      ng = branch_group(a->dtype, p.HS, p.N - g0, p.DV, kcap);
      BwdParams q = group(g0, ng);
      q.dv32 = multi ? a->dv_f32 : nullptr;
      if ((e = launch_attn_dkdv(a->dtype, q, st))) return status(e);
    }
  }
  return DTA_OK;
}

static int ln_common(const dta_ln_args* a, bool bwd) {
  if (!a || a->dtype < DTA_BF16 || a->dtype > DTA_F32 || a->rows < 0 || a->C <= 0) return DTA_ERR_INVALID;
  if (a->io_dtype != 0 && (a->dtype != DTA_F32 || (a->io_dtype - 1 != DTA_BF16 && a->io_dtype - 1 != DTA_F16)))
    return DTA_ERR_UNSUPPORTED;
  const int64_t v = 8;   // kernels move 8 elements per lane access
  if (a->C % v || a->C > 8192) return DTA_ERR_UNSUPPORTED;
  // no rows: nothing launches (launch_ln), nothing is read or written and dw / db keep what the
  // caller put there, so an empty tensor's NULL pointers are not an error
  if (a->rows == 0) return DTA_OK;
  if (!aligned_ptr(a->x) || a->x_stride % v || !a->w || !a->mean || !a->rstd) return DTA_ERR_INVALID;
  if (!bwd && (!aligned_ptr(a->y) || a->y_stride % v || !a->b)) return DTA_ERR_INVALID;
  if (bwd && (!aligned_ptr(a->dy) || !aligned_ptr(a->dx) || a->dy_stride % v || a->dx_stride % v || !a->dw || !a->db))
    return DTA_ERR_INVALID;
  // residual fusion: the mixed fp32 / 16-bit path only, with aligned 8-element rows
  const bool fused = bwd ? (a->dres || a->dx16) : (a->res || a->xo);
  if (fused && a->io_dtype == 0) return DTA_ERR_UNSUPPORTED;
  if (!bwd && fused && (!aligned_ptr(a->res) || !aligned_ptr(a->xo) || a->res_stride % v || a->xo_stride % v))
    return DTA_ERR_INVALID;
  if (bwd && a->partial && !aligned_ptr(a->partial)) return DTA_ERR_INVALID;   // 16-byte partial rows
  if (bwd && a->dres && (!aligned_ptr(a->dres) || a->dres_stride % v)) return DTA_ERR_INVALID;
  if (bwd && a->dx16 && (!aligned_ptr(a->dx16) || a->dx16_stride % v)) return DTA_ERR_INVALID;
  return DTA_OK;
}

static LnParams ln_params(const dta_ln_args* a) {
  LnParams p{};
  p.rows = a->rows; p.C = a->C; p.eps = a->eps; p.out_scale = a->out_scale;
  p.x = a->x; p.xs = a->x_stride; p.y = a->y; p.ys = a->y_stride;
  p.w = a->w; p.b = a->b; p.mean = a->mean; p.rstd = a->rstd;
  p.dy = a->dy; p.dys = a->dy_stride; p.dx = a->dx; p.dxs = a->dx_stride;
  p.dw = a->dw; p.db = a->db;
  p.partial = a->partial;
  p.res = a->res; p.ress = a->res_stride; p.xo = a->xo; p.xos = a->xo_stride;
  p.dres = a->dres; p.dress = a->dres_stride; p.dx16 = a->dx16; p.dx16s = a->dx16_stride;
  return p;
}

int dta_ln_fwd(const dta_ln_args* a, void* stream) {
  if (int e = ln_common(a, false)) return e;
  if (a->io_dtype) return status(launch_ln_mixed(a->io_dtype - 1, ln_params(a), false, (hipStream_t)stream));
  return status(launch_ln(a->dtype, ln_params(a), false, (hipStream_t)stream));
}

size_t dta_ln_bwd_workspace_bytes(int64_t rows, int64_t C) { return (size_t)ln_bwd_workspace_floats(rows, C) * 4; }

int dta_ln_bwd(const dta_ln_args* a, void* stream) {
  if (int e = ln_common(a, true)) return e;
  if (a->io_dtype) return status(launch_ln_mixed(a->io_dtype - 1, ln_params(a), true, (hipStream_t)stream));
  return status(launch_ln(a->dtype, ln_params(a), true, (hipStream_t)stream));
}

int dta_rope(const dta_rope_args* a, void* stream) {
  if (!a || !ok_dims(a->dtype, a->B, a->T, a->H, a->n_terms, a->head_size, 1)) return DTA_ERR_INVALID;
  if (a->head_size % 8) return DTA_ERR_UNSUPPORTED;
  if ((int64_t)a->B * a->T == 0) return DTA_OK;
  const int src_dtype = a->src_f32 ? DTA_F32 : a->dtype;
  // the kernel reads the freqs table by 16-byte vectors (as the attention entry points require)
  if (!ok_tensor(a->src, src_dtype, true) || !ok_tensor(a->dst, a->dtype, true) || !aligned_ptr(a->freqs))
    return DTA_ERR_INVALID;
  RopeParams p{};
  p.src = t5(a->src); p.dst = t5(a->dst); p.freqs = a->freqs;
  p.B = a->B; p.T = a->T; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.inverse = a->inverse ? 1 : 0;
  return status(launch_rope(a->dtype, a->src_f32 != 0, p, (hipStream_t)stream));
}

static int swiglu_common(const dta_swiglu_args* a, bool bwd, SwigluParams& p) {
  if (!a || a->dtype < DTA_BF16 || a->dtype > DTA_F32 || a->rows < 0 || a->n < 0) return DTA_ERR_INVALID;
  if (a->n % 8) return DTA_ERR_UNSUPPORTED;
  // no elements: nothing launches and no operand is read or written (an empty tensor's pointers
  // may be NULL); dta_swiglu_bwd still zeroes dbias
  const bool none = a->rows == 0 || a->n == 0;
  auto ok = [none](const void* q, int64_t st) { return (none || aligned_ptr(q)) && st % 8 == 0 && st >= 0; };
  if (!ok(a->a, a->a_stride) || !ok(a->b, a->b_stride)) return DTA_ERR_INVALID;
  if (!bwd && !ok(a->out, a->out_stride)) return DTA_ERR_INVALID;
  if (bwd && (!ok(a->dout, a->dout_stride) || !ok(a->da, a->da_stride) || !ok(a->db, a->db_stride)))
    return DTA_ERR_INVALID;
  p = SwigluParams{a->rows, a->n, a->a, a->a_stride, a->b, a->b_stride, a->out, a->out_stride,
                   a->dout, a->dout_stride, a->da, a->da_stride, a->db, a->db_stride};
  return DTA_OK;
}

int dta_swiglu_fwd(const dta_swiglu_args* a, void* stream) {
  SwigluParams p;
  if (int e = swiglu_common(a, false, p)) return e;
  return status(launch_swiglu(a->dtype, p, false, (hipStream_t)stream));
}

int dta_swiglu_bwd(const dta_swiglu_args* a, void* stream) {
  SwigluParams p;
  if (int e = swiglu_common(a, true, p)) return e;
  if (a->dbias) {
    if (!aligned_ptr(a->dbias) || !aligned_ptr(a->dbias_work)) return DTA_ERR_INVALID;
    if (a->rows == 0 || a->n == 0) return status(hipMemsetAsync(a->dbias, 0, sizeof(float) * 2 * a->n, (hipStream_t)stream));
    return status(launch_swiglu_bias(a->dtype, p, a->dbias, a->dbias_work, (hipStream_t)stream));
  }
  return status(launch_swiglu(a->dtype, p, true, (hipStream_t)stream));
}

size_t dta_swiglu_bwd_workspace_bytes(int64_t rows, int64_t n) {
  return rows < 0 || n < 0 ? 0 : (size_t)swiglu_bias_work_floats(rows, n) * 4;
}

int dta_accumulate_f32(int32_t dtype, int64_t n, const void* src, float* dst, void* stream) {
  if (dtype < DTA_BF16 || dtype > DTA_F32 || n < 0) return DTA_ERR_INVALID;
  if (n == 0) return DTA_OK;
  if (!aligned_ptr(src) || !aligned_ptr(dst)) return DTA_ERR_INVALID;
  return status(launch_accumulate(dtype, n, src, dst, (hipStream_t)stream));
}

int dta_cast_f32(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t n_terms, int32_t head_size,
                 const float* src, dta_tensor dst, void* stream) {
  if (!ok_dims(dtype, B, T, H, n_terms, head_size, 1) || head_size % 8) return DTA_ERR_INVALID;
  if ((int64_t)B * T == 0) return DTA_OK;
  if (!aligned_ptr(src) || !ok_tensor(dst, dtype, true)) return DTA_ERR_INVALID;
  return status(launch_cast(dtype, src, t5(dst), B, T, H, n_terms, head_size, (hipStream_t)stream));
}

static int64_t decode_splits(int32_t t_cap) { return (t_cap + DTA_DECODE_CHUNK - 1) / DTA_DECODE_CHUNK; }

size_t dta_attn_decode_workspace_bytes(int32_t B, int32_t H, int32_t n_terms, int32_t head_size, int32_t dv,
                                       int32_t t_cap) {
  const size_t single = (size_t)B * H * n_terms * t_cap * 4;
  const size_t split = (size_t)B * H * decode_splits(t_cap) * n_terms * (dv + 2) * 4;
  return single > split ? single : split;
}

// log2 of a page size the kernels take (32, 64, 128, 256), or 0 for any other
static int page_shift(int page_size) {
  switch (page_size) {
    case 32: return 5;
    case 64: return 6;
    case 128: return 7;
    case 256: return 8;
    default: return 0;
  }
}

// a device array of 4-byte elements (lengths, pos, count, a block table, a scale pool); NULL
// passes only where the argument is optional
static bool dev_i32(const void* p, bool required = true) { return (p || !required) && (uintptr_t)p % 4 == 0; }

// a multi-row step's own arguments: pos required, count optional
extern "C++" template <class A>
static bool step_ptrs_ok(const A* a) { return dev_i32(a->pos_dev) && dev_i32(a->count_dev, false); }

// The paged entry points' own arguments: a block table over a pool of n_pages pages of
// page_size rows, max_pages entries per sequence, t_cap the logical capacity.
extern "C++" template <class A>
static bool page_table(const A* a, PageTable& g) {
  if (!dev_i32(a->block_table_dev)) return false;
  const int shift = page_shift(a->page_size);
  if (!shift) return false;
  if (a->n_pages < 1 || a->max_pages < 1 || (int64_t)a->max_pages * a->page_size != a->t_cap) return false;
  g = PageTable{a->block_table_dev, a->max_pages, shift, a->n_pages};
  return true;
}

// a pool of e4m3fn bytes (strides in bytes): 16-byte pointer, page and row strides; heads and
// branches start on the widest load a lane makes of them (16 bytes, 8 where head_size % 16)
static bool ok_byte_pool(const dta_tensor& t, int width, bool with_i) {
  const int64_t v = width % 16 ? 8 : 16;
  if (!aligned_ptr(t.ptr) || t.sb % 16 || t.st % 16 || t.sh % v || (with_i && t.si % v)) return false;
  return t.sb >= 0 && t.st >= 0 && t.sh >= 0 && t.si >= 0;
}

// the fp8 entry points' own arguments, checked after the table: the scale pool, a page of it
// that holds every (row, head, K_i | V) scale, and 16-byte page and row strides of the byte pools
extern "C++" template <class A>
static bool fp8_scales_ok(const A* a) {
  if (!dev_i32(a->scale_pool_dev)) return false;
  if (a->H > 0 && a->n_terms > 0 && a->scale_page_stride < (int64_t)a->page_size * a->H * (a->n_terms + 1)) return false;
  return !(a->k_pool.sb % 16 || a->k_pool.st % 16 || a->v_pool.sb % 16 || a->v_pool.st % 16);
}

// q, o, coef and the cache views kc / vc (fp8: byte views) of every decode and extend entry point:
// each is read or written by 16-byte vector accesses (O of the extend by 8-byte ones)
extern "C++" template <class A>
static bool cache_operands_ok(const A* a, const dta_tensor& kc, const dta_tensor& vc, bool fp8) {
  if (!ok_tensor(a->q, a->dtype, true) || !ok_tensor(a->o, a->dtype, false) || !a->coef) return false;
  return fp8 ? ok_byte_pool(kc, a->head_size, true) && ok_byte_pool(vc, a->dv, false)
             : ok_tensor(kc, a->dtype, true) && ok_tensor(vc, a->dtype, false);
}

// What every decode launch takes, on checked operands.  kc / vc: the cache views (contiguous
// [b][t], or with a table in pg the page pool); scales: NULL, or the fp32 scale pool of an fp8 page
// pool; rows: query rows per (b, h); bound: the host bound of the keys, which sets the splits
extern "C++" template <class A>
static DecodeParams decode_params(const A* a, const dta_tensor& kc, const dta_tensor& vc, const PageTable& pg, int rows,
                                  int bound, const float* scales, int64_t scales_sb) {
  DecodeParams p{};
  p.q = t5(a->q); p.k = t5(kc); p.v = t5(vc); p.o = t5(a->o); p.pg = pg;
  p.coef = a->coef; p.ws = a->workspace;
  p.B = a->B; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.L = bound; p.ldw = a->t_cap; p.scale = a->scale;
  p.S = (int)decode_splits(bound);
  p.ml = a->workspace + (int64_t)a->B * a->H * rows * p.S * a->n_terms * a->dv;   // after the partial rows
  p.kvs = scales; p.kvs_sb = scales_sb;
  return p;
}

// the shared-prefix plan of dta_attn_decode_paged_shared and _fp8
struct SharedGroups { int n; const int32_t* members; const int32_t* rows; };

// Every one-row decode entry point: one validation, one launch path.  ldev / lsb: the device
// length(s) and their batch stride (0: one value, 1: int32 [B]); kc / vc / pg / scales as for
// decode_params; sh: NULL, or the plan, whose own checks follow the dims'
extern "C++" template <class A>
static int decode_call(const A* a, const dta_tensor& kc, const dta_tensor& vc, const int32_t* ldev, int lsb,
                       const PageTable& pg, void* stream, const float* scales = nullptr, int64_t scales_sb = 0,
                       const SharedGroups* sh = nullptr) {
  if (!ok_dims(a->dtype, a->B, 1, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  if (sh && (sh->n < 0 || (sh->n > 0 && (!dev_i32(sh->members) || !dev_i32(sh->rows))))) return DTA_ERR_INVALID;
  if (sh ? !decode_shared_supported(a->dtype, a->head_size, a->n_terms, a->dv)
         : a->head_size % 8 || a->head_size > 128 || a->n_terms > 4 || a->dv > 256)
    return DTA_ERR_UNSUPPORTED;
  if (a->length < 1 || a->t_cap < a->length) return DTA_ERR_INVALID;
  if ((int64_t)a->B * a->H == 0) return DTA_OK;
  if (!cache_operands_ok(a, kc, vc, scales != nullptr) || !aligned_ptr(a->workspace)) return DTA_ERR_INVALID;
  DecodeParams p = decode_params(a, kc, vc, pg, 1, a->length, scales, scales_sb);
  p.Ldev = ldev; p.Lsb = lsb;
  const hipStream_t st = (hipStream_t)stream;
  if (!sh) return status(scales ? launch_decode_f8(a->dtype, p, st) : launch_decode(a->dtype, p, st));
  p.sh_g = sh->n; p.sh_mem = sh->members; p.sh_rows = sh->rows;
  return status(scales ? launch_decode_shared_f8(a->dtype, p, st) : launch_decode_shared(a->dtype, p, st));
}

int dta_attn_decode(const dta_attn_decode_args* a, void* stream) {
  if (!a) return DTA_ERR_INVALID;
  return decode_call(a, a->k_cache, a->v_cache, a->length_dev, 0, PageTable{}, stream);
}

int dta_attn_decode_ragged(const dta_attn_decode_ragged_args* a, void* stream) {
  if (!a || !dev_i32(a->lengths_dev)) return DTA_ERR_INVALID;
  return decode_call(a, a->k_cache, a->v_cache, a->lengths_dev, 1, PageTable{}, stream);
}

int dta_attn_decode_paged(const dta_attn_decode_paged_args* a, void* stream) {
  PageTable pg{};
  if (!a || !dev_i32(a->lengths_dev) || !page_table(a, pg)) return DTA_ERR_INVALID;
  return decode_call(a, a->k_pool, a->v_pool, a->lengths_dev, 1, pg, stream);
}

int dta_attn_decode_paged_fp8(const dta_attn_decode_paged_fp8_args* a, void* stream) {
  PageTable pg{};
  if (!a || !dev_i32(a->lengths_dev) || !page_table(a, pg) || !fp8_scales_ok(a)) return DTA_ERR_INVALID;
  return decode_call(a, a->k_pool, a->v_pool, a->lengths_dev, 1, pg, stream, a->scale_pool_dev, a->scale_page_stride);
}

// ---- shared-prefix decode on the paged cache ----------------------------------------------------
int dta_decode_shared_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t fp8_cache) {
  (void)fp8_cache;   // every plan is built for 16-bit, 32-bit and e4m3 pages alike
  return decode_shared_supported(dtype, head_size, n_terms, dv) ? 1 : 0;
}

int dta_attn_decode_paged_shared(const dta_attn_decode_paged_shared_args* a, void* stream) {
  PageTable pg{};
  if (!a || !dev_i32(a->lengths_dev) || !page_table(a, pg)) return DTA_ERR_INVALID;
  const SharedGroups sh{a->n_groups, a->group_members_dev, a->group_rows_dev};
  return decode_call(a, a->k_pool, a->v_pool, a->lengths_dev, 1, pg, stream, nullptr, 0, &sh);
}

int dta_attn_decode_paged_shared_fp8(const dta_attn_decode_paged_shared_fp8_args* a, void* stream) {
  PageTable pg{};
  if (!a || !dev_i32(a->lengths_dev) || !page_table(a, pg) || !fp8_scales_ok(a)) return DTA_ERR_INVALID;
  const SharedGroups sh{a->n_groups, a->group_members_dev, a->group_rows_dev};
  return decode_call(a, a->k_pool, a->v_pool, a->lengths_dev, 1, pg, stream, a->scale_pool_dev, a->scale_page_stride,
                     &sh);
}

// ---- split-key decode for a step of 1 .. 8 rows per sequence -----------------------------------
int dta_decode_rows_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t Tq,
                              int32_t fp8_cache) {
  (void)fp8_cache;   // every plan is built for 16-bit, 32-bit and e4m3 caches alike
  return decode_rows_supported(dtype, head_size, n_terms, dv, Tq) ? 1 : 0;
}

size_t dta_attn_decode_rows_workspace_bytes(int32_t B, int32_t H, int32_t n_terms, int32_t head_size, int32_t dv,
                                            int32_t t_cap, int32_t Tq) {
  (void)head_size;
  if (B < 0 || H < 0 || n_terms < 0 || dv < 0 || t_cap < 0 || Tq < 0) return 0;
  return (size_t)B * H * Tq * decode_splits(t_cap) * n_terms * (dv + 2) * 4;
}

// dta_attn_decode_rows, _paged and _paged_fp8: the step's own checks (pos / count, the Tq range,
// the plan), then decode_call's of the operands and its launch parameters at the capacity
extern "C++" template <class A>
static int decode_rows_call(const A* a, const dta_tensor& kc, const dta_tensor& vc, const PageTable& pg, void* stream,
                            const float* scales = nullptr, int64_t scales_sb = 0) {
  if (!step_ptrs_ok(a)) return DTA_ERR_INVALID;
  if (a->Tq < 1 || a->Tq > 8) return DTA_ERR_INVALID;
  if (!ok_dims(a->dtype, a->B, a->Tq, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  if (!decode_rows_supported(a->dtype, a->head_size, a->n_terms, a->dv, a->Tq)) return DTA_ERR_UNSUPPORTED;
  if (a->t_cap < a->Tq) return DTA_ERR_INVALID;
  if ((int64_t)a->B * a->H == 0) return DTA_OK;
  if (!cache_operands_ok(a, kc, vc, scales != nullptr) || !aligned_ptr(a->workspace)) return DTA_ERR_INVALID;
  DecodeParams p = decode_params(a, kc, vc, pg, a->Tq, a->t_cap, scales, scales_sb);
  p.Tq = a->Tq; p.pos_dev = a->pos_dev; p.cnt_dev = a->count_dev;
  const hipStream_t st = (hipStream_t)stream;
  return status(scales ? launch_decode_rows_f8(a->dtype, p, st) : launch_decode_rows(a->dtype, p, st));
}

int dta_attn_decode_rows(const dta_attn_decode_rows_args* a, void* stream) {
  if (!a) return DTA_ERR_INVALID;
  return decode_rows_call(a, a->k_cache, a->v_cache, PageTable{}, stream);
}

int dta_attn_decode_rows_paged(const dta_attn_decode_rows_paged_args* a, void* stream) {
  PageTable pg{};
  if (!a || !page_table(a, pg)) return DTA_ERR_INVALID;
  return decode_rows_call(a, a->k_pool, a->v_pool, pg, stream);
}

int dta_attn_decode_rows_paged_fp8(const dta_attn_decode_rows_paged_fp8_args* a, void* stream) {
  PageTable pg{};
  if (!a || !page_table(a, pg) || !fp8_scales_ok(a)) return DTA_ERR_INVALID;
  return decode_rows_call(a, a->k_pool, a->v_pool, pg, stream, a->scale_pool_dev, a->scale_page_stride);
}

int dta_kv_quant_rows(const dta_kv_quant_rows_args* a, void* stream) {
  if (!a || !ok_dims(a->dtype, a->B, a->Tn, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  if (a->head_size % 16 || a->dv % 16 || a->head_size > 128 || a->dv > 256 || a->n_terms > 4)
    return DTA_ERR_UNSUPPORTED;
  const int shift = page_shift(a->page_size);
  if (!shift) return DTA_ERR_INVALID;
  if (a->n_pages < 1 || ((int64_t)a->n_pages + 1) * a->page_size > INT32_MAX) return DTA_ERR_INVALID;
  if (!dev_i32(a->slot_dev) || !dev_i32(a->scale_pool_dev) ||
      a->scale_page_stride < (int64_t)a->page_size * a->H * (a->n_terms + 1))
    return DTA_ERR_INVALID;
  if ((int64_t)a->B * a->Tn == 0) return DTA_OK;
  if (!ok_tensor(a->k_new, a->dtype, true) || !ok_tensor(a->v_new, a->dtype, false) ||
      !ok_byte_pool(a->k_pool, a->head_size, true) || !ok_byte_pool(a->v_pool, a->dv, false))
    return DTA_ERR_INVALID;
  KvQuantParams p{};
  p.ksrc = t5(a->k_new); p.vsrc = t5(a->v_new); p.kdst = t5(a->k_pool); p.vdst = t5(a->v_pool);
  p.kvs = a->scale_pool_dev; p.kvs_sb = a->scale_page_stride; p.slot = a->slot_dev;
  p.B = a->B; p.Tn = a->Tn; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.shift = shift; p.slots = (a->n_pages + 1) * a->page_size;
  return status(launch_kv_quant(a->dtype, p, (hipStream_t)stream));
}

int dta_kv_step_rows(const dta_kv_step_rows_args* a, void* stream) {
  if (!a || !ok_dims(a->dtype, a->B, a->Tn, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  if (a->head_size % 8 || a->dv % 8 || a->head_size > 128 || a->dv > 256 || a->n_terms > 8) return DTA_ERR_UNSUPPORTED;
  if (a->dest < DTA_KV_STEP_CONTIGUOUS || a->dest > DTA_KV_STEP_SLOTS) return DTA_ERR_INVALID;
  if (a->t_cap < 1 || a->t_cap > (1 << 30) || a->Tn > (1 << 30)) return DTA_ERR_INVALID;
  if (!dev_i32(a->pos_dev) || !dev_i32(a->count_dev)) return DTA_ERR_INVALID;
  const bool slots = a->dest == DTA_KV_STEP_SLOTS;
  int shift = 0;
  if (a->dest != DTA_KV_STEP_CONTIGUOUS) {
    shift = page_shift(a->page_size);
    if (!shift || a->n_pages < 1 || ((int64_t)a->n_pages + 1) * a->page_size > INT32_MAX || a->max_pages < 1 ||
        (int64_t)a->max_pages * a->page_size < a->t_cap)
      return DTA_ERR_INVALID;
    if (!dev_i32(a->block_table_dev)) return DTA_ERR_INVALID;
    if (slots && !dev_i32(a->slots_out_dev)) return DTA_ERR_INVALID;
  }
  if ((int64_t)a->B * a->Tn == 0) return DTA_OK;
  // every view is read or written by 16-byte vector accesses; the views a call does not use are not looked at
  const bool rope = a->rope_freqs != nullptr;
  if (rope && (!aligned_ptr(a->rope_freqs) || !ok_tensor(a->q, a->dtype, true) || !ok_tensor(a->q_out, a->dtype, true)))
    return DTA_ERR_INVALID;
  if ((rope || !slots) && (!ok_tensor(a->k, a->dtype, true) || !ok_tensor(a->k_dst, a->dtype, true))) return DTA_ERR_INVALID;
  if (!slots && (!ok_tensor(a->v, a->dtype, false) || !ok_tensor(a->v_dst, a->dtype, false))) return DTA_ERR_INVALID;
  KvStepParams p{};
  p.q = t5(a->q); p.k = t5(a->k); p.v = t5(a->v); p.qo = t5(a->q_out); p.kd = t5(a->k_dst); p.vd = t5(a->v_dst);
  p.freqs = a->rope_freqs; p.pos = a->pos_dev; p.cnt = a->count_dev; p.tbl = a->block_table_dev; p.slots = a->slots_out_dev;
  p.B = a->B; p.Tn = a->Tn; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.t_cap = a->t_cap; p.kind = a->dest; p.shift = shift; p.max_pages = a->max_pages; p.n_pages = a->n_pages;
  return status(launch_kv_step(a->dtype, p, (hipStream_t)stream));
}

// this library is built with -fno-honor-nans: x != x folds away, the bits do not
static bool nan_bits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x7fffffffu) > 0x7f800000u;
}

int dta_sample_rows(const dta_sample_rows_args* a, void* stream) {
  if (!a || a->dtype < DTA_BF16 || a->dtype > DTA_F32 || a->R < 0 || a->V < 1) return DTA_ERR_INVALID;
  if (nan_bits(a->temperature) || nan_bits(a->top_p)) return DTA_ERR_INVALID;
  if ((uintptr_t)a->temperature_dev % 4 || (uintptr_t)a->top_k_dev % 4 || (uintptr_t)a->top_p_dev % 4 ||
      (uintptr_t)a->logprob_out % 4 || (uintptr_t)a->stream_dev % 8 || (uintptr_t)a->offset_dev % 8 ||
      (uintptr_t)a->token_out % 8)
    return DTA_ERR_INVALID;
  if (a->V > (1 << 20)) return DTA_ERR_UNSUPPORTED;
  if (a->R == 0) return DTA_OK;
  if (!a->logits || !a->token_out || (uintptr_t)a->logits % (a->dtype == DTA_F32 ? 4 : 2)) return DTA_ERR_INVALID;
  SampleParams p{};
  p.logits = a->logits; p.stride = a->row_stride; p.R = a->R; p.V = a->V;
  p.T = a->temperature; p.k = a->top_k; p.p = a->top_p;
  p.Tdev = a->temperature_dev; p.kdev = a->top_k_dev; p.pdev = a->top_p_dev;
  p.seed = a->seed; p.strm = a->stream_dev; p.off = a->offset_dev; p.tok = a->token_out; p.lp = a->logprob_out;
  return status(launch_sample(a->dtype, p, (hipStream_t)stream));
}

size_t dta_penalize_rows_workspace_bytes(int64_t R, int32_t V) {
  if (R < 0 || V < 1 || V > (1 << 20)) return 0;
  return penalize_workspace_bytes(R, V);
}

int dta_penalize_rows(const dta_penalize_rows_args* a, void* stream) {
  if (!a || a->dtype < DTA_BF16 || a->dtype > DTA_F32 || a->B < 0 || a->Tn < 0 || a->V < 1) return DTA_ERR_INVALID;
  const int64_t R = (int64_t)a->B * a->Tn;
  if (R > INT32_MAX || a->cap < 1 || a->cap > (1 << 30) || a->K < 0 || a->K > 7) return DTA_ERR_INVALID;
  if (a->row_stride < a->V || a->out_stride < a->V || a->hist_stride < a->cap) return DTA_ERR_INVALID;
  if ((a->draft == nullptr) != (a->dcnt_dev == nullptr) || (a->draft && a->draft_stride < a->K)) return DTA_ERR_INVALID;
  if (a->bias && a->bias_stride != 0 && a->bias_stride < a->V) return DTA_ERR_INVALID;
  if (nan_bits(a->repetition) || nan_bits(a->frequency) || nan_bits(a->presence) || nan_bits(a->floor_gap) ||
      a->repetition <= 0.f)
    return DTA_ERR_INVALID;
  if (!dev_i32(a->out, false) || !dev_i32(a->hist, false) || !dev_i32(a->hlen_dev, false) ||
      !dev_i32(a->gen_start_dev, false) || !dev_i32(a->draft, false) || !dev_i32(a->dcnt_dev, false) ||
      !dev_i32(a->repetition_dev, false) || !dev_i32(a->frequency_dev, false) || !dev_i32(a->presence_dev, false) ||
      !dev_i32(a->floor_gap_dev, false) || !dev_i32(a->bias, false) || !dev_i32(a->workspace, false) ||
      (uintptr_t)a->logits % esize(a->dtype))
    return DTA_ERR_INVALID;
  if (a->V > (1 << 20)) return DTA_ERR_UNSUPPORTED;
  if (R == 0) return DTA_OK;
  if (!a->logits || !a->out || !a->hist || !a->hlen_dev) return DTA_ERR_INVALID;
  const size_t need = penalize_workspace_bytes(R, a->V);
  if (need && (!a->workspace || a->workspace_bytes < need)) return DTA_ERR_INVALID;
  PenaltyParams p{};
  p.logits = a->logits; p.out = a->out; p.stride = a->row_stride; p.out_stride = a->out_stride;
  p.hist = a->hist; p.hlen = a->hlen_dev; p.gen_start = a->gen_start_dev; p.draft = a->draft; p.dcnt = a->dcnt_dev;
  p.hist_stride = a->hist_stride; p.draft_stride = a->draft_stride;
  p.theta = a->repetition; p.freq = a->frequency; p.pres = a->presence; p.gap = a->floor_gap;
  p.theta_dev = a->repetition_dev; p.freq_dev = a->frequency_dev; p.pres_dev = a->presence_dev; p.gap_dev = a->floor_gap_dev;
  p.bias = a->bias; p.bias_stride = a->bias_stride; p.ws = need ? static_cast<uint32_t*>(a->workspace) : nullptr;
  p.R = (int)R; p.Tn = a->Tn; p.V = a->V; p.cap = a->cap; p.K = a->K;
  return status(launch_penalize(a->dtype, p, (hipStream_t)stream));
}

int dta_spec_accept_draft(const dta_spec_accept_draft_args* a, void* stream) {
  if (!a || a->B < 0 || a->K < 1 || a->K > 7 || a->Tn < 0 || a->Tn > a->K + 1) return DTA_ERR_INVALID;
  if (a->ngram_min < 0 || a->ngram_min > a->ngram_max || a->ngram_max < 1 || a->ngram_max > 8) return DTA_ERR_INVALID;
  if (a->cap < 1 || a->cap > (1 << 30) || a->t_cap < 1 || a->t_cap > (1 << 30)) return DTA_ERR_INVALID;
  if (a->hist_stride < a->cap || a->draft_stride < a->K || a->tok_stride < a->Tn) return DTA_ERR_INVALID;
  if (!a->hist || !a->hlen_dev || !a->remaining_dev || !a->draft || !a->dcnt_dev || !a->result_out ||
      (a->Tn > 0 && !a->tok))
    return DTA_ERR_INVALID;
  if ((uintptr_t)a->hist % 4 || (uintptr_t)a->hlen_dev % 4 || (uintptr_t)a->remaining_dev % 4 || (uintptr_t)a->draft % 4 ||
      (uintptr_t)a->dcnt_dev % 4 || (uintptr_t)a->result_out % 4 || (uintptr_t)a->tok % 8)
    return DTA_ERR_INVALID;
  if (a->B == 0) return DTA_OK;
  SpecParams p{};
  p.hist = a->hist; p.hlen = a->hlen_dev; p.remaining = a->remaining_dev; p.draft = a->draft; p.dcnt = a->dcnt_dev;
  p.tok = a->tok; p.result = a->result_out;
  p.hist_stride = a->hist_stride; p.draft_stride = a->draft_stride; p.tok_stride = a->tok_stride;
  p.B = a->B; p.Tn = a->Tn; p.K = a->K; p.cap = a->cap; p.t_cap = a->t_cap;
  p.nmin = a->ngram_min; p.nmax = a->ngram_max; p.eos = a->eos_id;
  return status(launch_spec(p, (hipStream_t)stream));
}

int dta_spec_feed_rows(const dta_spec_feed_rows_args* a, void* stream) {
  if (!a || a->B < 0 || a->K < 1 || a->K > 7 || a->vocab < 1 || a->total < 0) return DTA_ERR_INVALID;
  if (a->cap < 1 || a->cap > (1 << 30)) return DTA_ERR_INVALID;
  if (a->hist_stride < a->cap || a->draft_stride < a->K || a->idx_stride < a->K + 1 || a->offset_stride < a->K + 1)
    return DTA_ERR_INVALID;
  if (!a->hist || !a->hlen_dev || !a->remaining_dev || !a->draft || !a->dcnt_dev || !a->idx_out || !a->counts_out ||
      !a->offset_out)
    return DTA_ERR_INVALID;
  if ((uintptr_t)a->hist % 4 || (uintptr_t)a->hlen_dev % 4 || (uintptr_t)a->remaining_dev % 4 || (uintptr_t)a->draft % 4 ||
      (uintptr_t)a->dcnt_dev % 4 || (uintptr_t)a->counts_out % 4 || (uintptr_t)a->idx_out % 8 || (uintptr_t)a->offset_out % 8)
    return DTA_ERR_INVALID;
  if (a->B == 0) return DTA_OK;
  SpecFeedParams p{};
  p.hist = a->hist; p.hlen = a->hlen_dev; p.remaining = a->remaining_dev; p.draft = a->draft; p.dcnt = a->dcnt_dev;
  p.idx = a->idx_out; p.counts = a->counts_out; p.offset = a->offset_out;
  p.hist_stride = a->hist_stride; p.draft_stride = a->draft_stride; p.idx_stride = a->idx_stride;
  p.offset_stride = a->offset_stride;
  p.B = a->B; p.K = a->K; p.cap = a->cap; p.vocab = a->vocab; p.total = a->total;
  return status(launch_spec_feed(p, (hipStream_t)stream));
}

int dta_spec_commit_lengths(const dta_spec_commit_lengths_args* a, void* stream) {
  if (!a || a->B < 0 || a->K < 1 || a->K > 7 || a->t_cap < 1 || a->t_cap > (1 << 30) || a->n_slots < 1)
    return DTA_ERR_INVALID;
  if (!a->slots && a->n_slots < a->B) return DTA_ERR_INVALID;
  if (!a->lengths || !a->result) return DTA_ERR_INVALID;
  if ((uintptr_t)a->lengths % 4 || (uintptr_t)a->result % 4 || (uintptr_t)a->slots % 8) return DTA_ERR_INVALID;
  if (a->B == 0) return DTA_OK;
  SpecCommitParams p{};
  p.lengths = a->lengths; p.result = a->result; p.slots = a->slots;
  p.B = a->B; p.K = a->K; p.t_cap = a->t_cap; p.n_slots = a->n_slots;
  return status(launch_spec_commit(p, (hipStream_t)stream));
}

int dta_extend_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv) {
  return extend_supported(dtype, head_size, n_terms, dv) ? 1 : 0;
}

int dta_extend_fp8_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv) {
  return extend_f8_supported(dtype, head_size, n_terms, dv) ? 1 : 0;
}

// Every extend entry point: one validation, one launch path.  pos: the host position of
// dta_attn_extend; pos_dev / cnt_dev: the ragged forms'; kc / vc / pg / scales as for decode_params
extern "C++" template <class A>
static int extend_call(const A* a, const dta_tensor& kc, const dta_tensor& vc, int pos, const int32_t* pos_dev,
                       const int32_t* cnt_dev, const PageTable& pg, void* stream, const float* scales = nullptr,
                       int64_t scales_sb = 0) {
  if (!ok_dims(a->dtype, a->B, a->Tq, a->H, a->n_terms, a->head_size, a->dv)) return DTA_ERR_INVALID;
  if (scales ? !extend_f8_supported(a->dtype, a->head_size, a->n_terms, a->dv)
             : !extend_supported(a->dtype, a->head_size, a->n_terms, a->dv))
    return DTA_ERR_UNSUPPORTED;
  if (pos < 0 || a->t_cap < 0 || (int64_t)pos + a->Tq > a->t_cap) return DTA_ERR_INVALID;
  if (a->Tq == 0 || (int64_t)a->B * a->H == 0) return DTA_OK;
  if (!cache_operands_ok(a, kc, vc, scales != nullptr)) return DTA_ERR_INVALID;
  ExtendParams p{};
  p.q = t5(a->q); p.k = t5(kc); p.v = t5(vc); p.o = t5(a->o); p.pg = pg;
  p.coef = a->coef;
  p.B = a->B; p.H = a->H; p.N = a->n_terms; p.HS = a->head_size; p.DV = a->dv;
  p.Tq = a->Tq; p.pos = pos; p.sl2 = a->scale * kLog2e;
  p.pos_dev = pos_dev; p.cnt_dev = cnt_dev; p.cap = a->t_cap;
  p.kvs = scales; p.kvs_sb = scales_sb;
  const hipStream_t st = (hipStream_t)stream;
  return status(scales ? launch_extend_f8(a->dtype, p, st) : launch_extend(a->dtype, p, st));
}

int dta_attn_extend(const dta_attn_extend_args* a, void* stream) {
  if (!a) return DTA_ERR_INVALID;
  return extend_call(a, a->k_cache, a->v_cache, a->pos, nullptr, nullptr, PageTable{}, stream);
}

int dta_attn_extend_ragged(const dta_attn_extend_ragged_args* a, void* stream) {
  if (!a || !step_ptrs_ok(a)) return DTA_ERR_INVALID;
  return extend_call(a, a->k_cache, a->v_cache, 0, a->pos_dev, a->count_dev, PageTable{}, stream);
}

int dta_attn_extend_paged(const dta_attn_extend_paged_args* a, void* stream) {
  PageTable pg{};
  if (!a || !step_ptrs_ok(a) || !page_table(a, pg)) return DTA_ERR_INVALID;
  return extend_call(a, a->k_pool, a->v_pool, 0, a->pos_dev, a->count_dev, pg, stream);
}

int dta_attn_extend_paged_fp8(const dta_attn_extend_paged_fp8_args* a, void* stream) {
  PageTable pg{};
  if (!a || !step_ptrs_ok(a) || !page_table(a, pg) || !fp8_scales_ok(a)) return DTA_ERR_INVALID;
  return extend_call(a, a->k_pool, a->v_pool, 0, a->pos_dev, a->count_dev, pg, stream, a->scale_pool_dev,
                     a->scale_page_stride);
}

}  // extern "C"
