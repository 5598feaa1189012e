// dta_internal.h -- host-side parameter blocks shared between the C-ABI
// (capi.hip) and the per-dtype kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dta {

struct T5 {            // [b][t][h][i] element strides + base pointer
  void* p;
  int64_t sb, st, sh, si;
};

struct FwdParams {
  T5 q, k, v, o, obr;
  float* lse;
  const float* coef;
  int B, T, H, N, HS, DV;
  float sl2;           // scale * log2(e)
  unsigned long long* stamps;   // diagnostic builds (DTA_STAMPS) only: per-wave segment cycle sums
  uint32_t drop_thr;   // attention dropout: keep iff hash >= drop_thr (= p * 2^32); 0 = off
  float drop_scale;    // 1 / (1 - p)
  uint32_t drop_seed_lo, drop_seed_hi;
  int bsplit;          // launcher-internal: > 1 = branch-split launch of the N = 1 kernel
                       // (one branch of bsplit per workgroup; writes O_i and LSE_i only)
  int bseq;            // launcher-internal: > 1 = the N = 1 kernel runs bseq branches one after
                       // another per workgroup and writes O as well (no combine pass)
  int cst;             // row stride of coef [h][cst] (the call's total branch count)
  const float* rope;   // if set (ABI 5): q is un-rotated; the forward rotates Q_i at load
  T5 qrot;             //   (fp32 [T][HS/2][2] table) and stores the rotated rows here
  int ob16;            // O_i (obr) stored as fp16 instead of fp32 (ABI 6, 16-bit activations)
};

struct BwdParams {
  T5 q, k, v, obr, dout, dq, dk, dv;
  const float* lse;
  float* delta;        // written by attn_dq, read by attn_dkdv
  const float* coef;
  float* dcoef;        // accumulated by attn_dq (zeroed first)
  float* dq32;         // if set: dQ written as fp32 [b][t][h][i][d] instead of into dq
  const float* rope;   // if set: fp32 [T][HS/2][2] table; dQ / dK leave through the inverse rotation
  float* dcoef_part;   // if set: per-wave d(coef) partials [h][i][b][T/32] (no atomics), summed by dcoef_reduce
  int B, T, H, N, HS, DV;
  float sl2, scale;
  unsigned long long* stamps;   // as FwdParams::stamps
  uint32_t drop_thr;   // as FwdParams
  float drop_scale;
  uint32_t drop_seed_lo, drop_seed_hi;
  // branch groups (capi: a call whose N has no kernel plan runs as groups of branches
  // that have one; every branch-indexed pointer above is then offset to the group's
  // first branch br0):
  int cst;             // the call's total branch count: row stride of coef / dcoef
                       // [h][cst], of the d(coef) partials and of dq32; dropout's branch index
  int br0;             // the group's first branch (dropout mask key)
  int dv_acc;          // dK/dV kernel: add into dv instead of storing (groups after the first)
  float* dv32;         // optional fp32 [b][t][h][e] running dV sum across branch groups
  int dv_last;         // the last dK/dV group (with dv32: the one that writes dv)
  int ob16;            // obr holds fp16 O_i (ABI 6)
  float* lsec;         // optional (ABI 8 lse_c, 16-bit, no dropout): stored LSE_i + log2|c_i| rows
                       // [i][b][h][t], written by attn_dq, the S seeds of attn_dkdv (|c_i| folded into P)
  uint64_t kstarts;    // attn_dq run as one group, no dropout: the dK/dV grouping's starts (bit i), so the
                       // delta rows are written in that encoding and no rebase launch follows (0: own group)
};

// per-dtype launchers (dtype index: 0 bf16, 1 f16, 2 f32); return hipError_t
int launch_attn_fwd(int dtype, const FwdParams& p, hipStream_t st);
// dropout instantiations (attn_*_drop.hip): the same kernels with the mask compiled in
int launch_attn_fwd_drop(int dtype, const FwdParams& p, hipStream_t st);
int launch_attn_dq_drop(int dtype, const BwdParams& p, hipStream_t st);
int launch_attn_dkdv_drop(int dtype, const BwdParams& p, hipStream_t st);
int launch_attn_dq(int dtype, const BwdParams& p, hipStream_t st);
int launch_attn_dkdv(int dtype, const BwdParams& p, hipStream_t st);
bool attn_supported(int dtype, int hs, int n, int dv);   // any kernel path: native plan or branch groups
bool attn_native(int dtype, int hs, int n, int dv);      // an N-branch kernel plan is built

struct LnParams {
  int64_t rows, C;
  float eps, out_scale;
  const void* x; int64_t xs;
  void* y; int64_t ys;
  const float* w; const float* b;
  float* mean; float* rstd;
  const void* dy; int64_t dys;
  void* dx; int64_t dxs;
  float* dw; float* db;
  float* partial;      // optional [blocks][2][C] workspace: deterministic dw/db (no atomics)
  // residual fusion (mixed fp32 x / 16-bit y path only; NULL = off):
  const void* res; int64_t ress;   // fwd: x + res (res in y's dtype) is normalised ...
  float* xo; int64_t xos;          // ... and written here (fp32)
  const float* dres; int64_t dress;  // bwd: dx += dres (the residual branch's gradient)
  void* dx16; int64_t dx16s;       // bwd: dx also stored in y's dtype
};
int launch_ln_mixed(int y_dtype, const LnParams& p, bool bwd, hipStream_t st);   // x fp32, y / dy 16-bit
int ln_bwd_blocks(int64_t rows);
int64_t ln_bwd_workspace_floats(int64_t rows, int64_t C);

struct RopeParams {
  T5 src, dst;
  const float* freqs;
  int B, T, H, N, HS;
  int inverse;
};

#ifndef DTA_DECODE_CHUNK
#define DTA_DECODE_CHUNK 256   // keys per workgroup of the split-key decode plan
#endif

// Paged caches (dta_attn_decode_paged / dta_attn_extend_paged): k / v describe a pool of
// pages ([page][row < 2^shift][h][i]: sb = page stride, st = row stride) and row j of
// sequence b lives at pool[tbl[b * max_pages + (j >> shift)]][j & (2^shift - 1)].
// tbl == NULL: the contiguous cache ([b][t][h][i]) of every other entry point.
struct PageTable {
  const int* tbl;      // device int32 [B][max_pages]
  int max_pages;       // table row length
  int shift;           // log2(page size): 5 .. 8
  int n_pages;         // pages of the pool: every id read from tbl is clamped to [0, n_pages - 1]
};
// the pool page that holds row j of sequence b, clamped so that no device value can index
// outside the pool (as clamp_len and the pos_b clamp do for lengths and positions)
__device__ __forceinline__ int page_of(const PageTable& g, int b, int j) {
  return min(max(g.tbl[(int64_t)b * g.max_pages + (j >> g.shift)], 0), g.n_pages - 1);
}

struct DecodeParams {
  T5 q, k, v, o;       // q/o: one row per (b, h) (st unused); k/v: the cache [b][t][h][i]
  const float* coef;   // [h][i]
  float* ws;           // single pass: fp32 [b][h][i][ldw]; split: partial rows [b][h][s][i][DV]
  float* ml;           // split path: fp32 [b][h][s][i][2] chunk (max, sum); null = single pass
  int B, H, N, HS, DV, L, ldw, S;   // L: length, or its upper bound when Ldev is set
  float scale;
  const int* Ldev;     // optional device length
  int Lsb;             // batch stride of Ldev: 0 = one length for the launch, 1 = int32 [B] (ragged)
  PageTable pg;        // paged launch: k / v are the page pool, ldw = max_pages * page size
  // fp8 cache (dta_attn_decode_paged_fp8; NULL otherwise): k / v are pools of e4m3fn bytes (strides
  // in bytes) and kvs the fp32 scales [page][row < P][h][N + 1] (index N: V), kvs_sb floats per page
  const float* kvs;
  int64_t kvs_sb;
  // several query rows per launch (dta_attn_decode_rows*; pos_dev NULL otherwise): q / o hold Tq rows
  // per (b, h) (st used), row r is the one-row decode at length pos_b + r + 1; L = ldw = the capacity,
  // ws the partial rows [b][h][r][s][i][DV], ml [b][h][r][s][i][2]
  int Tq;              // 1 .. 8
  const int* pos_dev;  // int32 [B]: sequence b's pos, clamped to [0, ldw - Tq]
  const int* cnt_dev;  // optional int32 [B]: real rows of sequence b, clamped to [0, Tq]; rows past it are written as zeros
  // shared-prefix plan (dta_attn_decode_paged_shared*; sh_mem NULL otherwise): sh_g groups of up to 8
  // sequences whose cache rows 0 .. sh_rows[g] - 1 are the same pool pages; the group pass reads those
  // rows once per group and the one-row pass of that step skips the chunks it covered
  int sh_g;
  const int* sh_mem;   // int32 [sh_g][8]: batch indices, anything outside [0, B) is an empty slot
  const int* sh_rows;  // int32 [sh_g]: shared rows, clamped to [0, the shortest member's length]
};

int launch_decode(int dtype, const DecodeParams& p, hipStream_t st);
// paged / fp8-paged one-row decode under a shared-prefix plan: split plan only; -2 without one
int launch_decode_shared(int dtype, const DecodeParams& p, hipStream_t st);
int launch_decode_shared_f8(int dtype, const DecodeParams& p, hipStream_t st);
bool decode_shared_supported(int dtype, int hs, int n, int dv);
int launch_decode_f8(int dtype, const DecodeParams& p, hipStream_t st);   // dtype: q / o; cache rows fp8
int launch_decode_rows(int dtype, const DecodeParams& p, hipStream_t st);      // split plan only; -2 without one
int launch_decode_rows_f8(int dtype, const DecodeParams& p, hipStream_t st);
bool decode_rows_supported(int dtype, int hs, int n, int dv, int tq);

// dta_kv_quant_rows (kv_quant.hip): rows of K_i / V in the activation dtype -> e4m3fn bytes + scales
struct KvQuantParams {
  T5 ksrc, vsrc;       // [b][t][h][i][d] / [b][t][h][e], activation dtype, element strides
  T5 kdst, vdst;       // byte pools [page][row < P][h][i][d] / [page][row < P][h][e], byte strides
  float* kvs;          // scale pool [page][row < P][h][N + 1]
  int64_t kvs_sb;      // floats per scale page
  const int* slot;     // device int32 [B * Tn]: page * P + row, clamped to [0, slots - 1]
  int B, Tn, H, N, HS, DV;
  int shift;           // log2(page size)
  int slots;           // (n_pages + 1) * P: the pool's pages and the spare page after them
};
int launch_kv_quant(int dtype, const KvQuantParams& p, hipStream_t st);

// dta_kv_step_rows (kv_step.hip): the RoPE and the cache scatter of a step's rows at per-sequence positions
struct KvStepParams {
  T5 q, k, v;          // the step's rows [b][t < Tn][h][i][d] / [b][t < Tn][h][e], element strides
  T5 qo;               // rotated Q_i, as q (freqs set)
  T5 kd, vd;           // by kind: the cache [b][t_cap], the pool [page][row < P], or kd = k_out as k (vd unused)
  const float* freqs;  // the whole fp32 [t_cap][HS/2][2] table, or NULL: no rotation, q is not touched
  const int* pos;      // device int32 [B], clamped to [0, t_cap]
  const int* cnt;      // device int32 [B]: real rows of sequence b
  const int* tbl;      // paged / slots: device int32 [B][max_pages]; every id read is clamped to [0, n_pages - 1]
  int* slots;          // slots: device int32 [B * Tn] out
  int B, Tn, H, N, HS, DV;
  int t_cap, kind;     // kind: dta_kv_step_dest
  int shift, max_pages, n_pages;   // shift: log2(page size), 0 for the contiguous cache
};
int launch_kv_step(int dtype, const KvStepParams& p, hipStream_t st);

// dta_sample_rows (sample.hip): one token per logits row, seeded temperature / top-k / top-p sampling
struct SampleParams {
  const void* logits;  // [R][V] in the launch's dtype, row stride in elements
  int64_t stride;
  int R, V;
  float T; int k; float p;                     // used where the per-row pointer is NULL
  const float* Tdev; const int* kdev; const float* pdev;
  uint64_t seed;
  const int64_t* strm; // [R] or NULL: the row index
  const int64_t* off;  // [R] or NULL: 0
  int64_t* tok;        // [R]
  float* lp;           // [R] or NULL
};
int launch_sample(int dtype, const SampleParams& p, hipStream_t st);

// dta_penalize_rows (penalty.hip): penalties, bias and the min-p floor of logits rows into fp32 rows
struct PenaltyParams {
  const void* logits;  // [R][V] in the launch's dtype, row stride in elements
  float* out;          // [R][V] fp32
  int64_t stride, out_stride;
  const int* hist;     // [B][cap], row stride in elements
  const int* hlen;     // [B], clamped to [0, cap]
  const int* gen_start;  // [B] or NULL: 0; clamped to [0, hlen]
  const int* draft;    // [B][K] or NULL
  const int* dcnt;     // [B] with draft, clamped to [0, K]
  int64_t hist_stride, draft_stride;
  float theta, freq, pres, gap;                // used where the per-sequence pointer is NULL
  const float* theta_dev; const float* freq_dev; const float* pres_dev; const float* gap_dev;
  const float* bias;   // [B][V] or, bias_stride 0, [V]; or NULL
  int64_t bias_stride;
  uint32_t* ws;        // [R][V] where V is past the LDS table, not read before it is written
  int R, Tn, V, cap, K;
};
int launch_penalize(int dtype, const PenaltyParams& p, hipStream_t st);
size_t penalize_workspace_bytes(int64_t R, int64_t V);

// dta_spec_accept_draft (spec.hip): a speculative round's acceptance, history append and next n-gram draft
struct SpecParams {
  int* hist;           // [B][cap], row stride in elements
  int* hlen;           // [B], clamped to [0, cap]
  int* remaining;      // [B]; <= 0: a finished row
  int* draft;          // [B][K]
  int* dcnt;           // [B], clamped to [0, min(K, Tn - 1)]
  const int64_t* tok;  // [B][Tn]
  int* result;         // [B][2]: (m, next dcnt)
  int64_t hist_stride, draft_stride, tok_stride;
  int B, Tn, K, cap, t_cap, nmin, nmax, eos;   // nmin 0: no lookup, the next dcnt is 0
};
int launch_spec(const SpecParams& p, hipStream_t st);

// dta_spec_feed_rows (spec_round.hip): a fixed-shape round's tokens, counts and sampler offsets
struct SpecFeedParams {
  const int* hist;       // [B][cap], row stride in elements
  const int* hlen;       // [B], clamped to [0, cap]
  const int* remaining;  // [B]; <= 0: a finished row
  const int* draft;      // [B][K]
  const int* dcnt;       // [B], clamped to [0, K]
  int64_t* idx;          // [B][K + 1]
  int* counts;           // [B]
  int64_t* offset;       // [B][K + 1]
  int64_t hist_stride, draft_stride, idx_stride, offset_stride;
  int B, K, cap, vocab, total;
};
int launch_spec_feed(const SpecFeedParams& p, hipStream_t st);

// dta_spec_commit_lengths (spec_round.hip): lengths[slot] += the round's emitted tokens
struct SpecCommitParams {
  int* lengths;          // [n_slots]
  const int* result;     // [B][2]
  const int64_t* slots;  // [B] or null, clamped to [0, n_slots - 1]
  int B, K, t_cap, n_slots;
};
int launch_spec_commit(const SpecCommitParams& p, hipStream_t st);

struct ExtendParams {
  T5 q, k, v, o;       // q/o: Tq rows per (b, h); k/v: the cache [b][t][h][i], rows 0 .. pos+Tq-1 valid
  const float* coef;   // [h][i]
  int B, H, N, HS, DV;
  int Tq, pos;         // query row r sits at absolute position pos + r
  float sl2;           // scale * log2(e)
  // ragged batches (dta_attn_extend_ragged; both NULL = the one-position launch above)
  const int* pos_dev;  // int32 [B]: sequence b's pos, clamped to [0, cap - Tq]
  const int* cnt_dev;  // optional int32 [B]: real rows of sequence b, clamped to [0, Tq]; rows past it are written as zeros
  int cap;             // rows of the cache views (the clamp of pos_dev); paged: max_pages * page size
  PageTable pg;        // paged launch: k / v are the page pool
  // fp8 cache (dta_attn_extend_paged_fp8; NULL otherwise): as DecodeParams' kvs / kvs_sb
  const float* kvs;
  int64_t kvs_sb;
};

int launch_extend(int dtype, const ExtendParams& p, hipStream_t st);   // extend.hip
bool extend_supported(int dtype, int hs, int n, int dv);
int launch_extend_f8(int dtype, const ExtendParams& p, hipStream_t st);   // dtype: q / o; cache rows fp8
bool extend_f8_supported(int dtype, int hs, int n, int dv);
int launch_ln(int dtype, const LnParams& p, bool bwd, hipStream_t st);
int launch_rope(int dtype, bool src_f32, const RopeParams& p, hipStream_t st);
int launch_dcoef_reduce(const float* part, float* dcoef, int H, int N, int64_t per, hipStream_t st);
int launch_delta_rebase(float* delta, int64_t rows, int N, uint64_t from, uint64_t to, hipStream_t st);
int launch_cast(int dtype, const float* src, const T5& dst, int B, int T, int H, int N, int HS, hipStream_t st);

struct SwigluParams {
  int64_t rows, n;                       // rows x n elements, n % 8 == 0
  const void* a; int64_t as;             // gate pre-activation (row stride, elements)
  const void* b; int64_t bs;             // linear branch
  void* out; int64_t os;                 // forward output
  const void* dout; int64_t dos;         // backward: incoming gradient
  void* da; int64_t das;
  void* db; int64_t dbs;
};
int launch_swiglu(int dtype, const SwigluParams& p, bool bwd, hipStream_t st);
int launch_accumulate(int dtype, int64_t n, const void* src, float* dst, hipStream_t st);
int launch_swiglu_bias(int dtype, const SwigluParams& p, float* dbias, float* work, hipStream_t st);
int64_t swiglu_bias_work_floats(int64_t rows, int64_t n);

}  // namespace dta
