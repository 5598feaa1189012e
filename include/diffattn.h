/*
 * diffattn.h -- C ABI of libdiffattn.so, the MI355X (gfx950) differential
 * attention library.
 *
 * The reference (JoshFCooper415/differential_transformer_replication) has no
 * native code, plugin or FFI: its hot path is eager ATen called from
 * nn.Module.forward.  Each entry point below replaces a group of those eager
 * ops; the comment on each cites the reference lines it replaces.  The Python
 * package binds these through ctypes (differential_transformer_replication_amd/
 * _lib.py); INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - Plain C types only: device pointers, element strides (int64, in
 *    ELEMENTS not bytes), sizes, a hipStream_t passed as void*.
 *  - The caller (PyTorch's caching allocator) owns every buffer.  The library
 *    never allocates or frees device memory and keeps no state.
 *  - Every launch is asynchronous on the given stream; no host sync.
 *  - Functions return DTA_OK (0) or a negative error code and never throw
 *    across the ABI; dta_error_string() describes a code.
 *  - dtype applies to Q/K/V/O/dO/dQ/dK/dV activations; Obr, LSE, delta, the
 *    coefficients, the LayerNorm statistics/parameters and every *_f32 buffer
 *    are always fp32.
 *
 * Layouts (element strides are given per tensor so strided views of one
 * packed projection output can be passed without copies):
 *   Q, K   [b][t][h][i][d]   i < n_terms (the N softmax branches), d < head_size
 *   V, O   [b][t][h][e]      e < dv (dv = 2*head_size for diff attention; dv = head_size with n_terms = 1
 *                             for standard attention, head_size 64 or 128)
 *   Obr    [i][b][t][h][e]   per-branch normalised outputs A_i V, fp32 (default) or fp16
 *                             (obr_dtype, 16-bit activations only); saved for bwd:
 *                             delta_i = <dO, O_i> and d(coef) come from them
 *   LSE    [i][b][h][t]      fp32, NEGATED log2-sum-exp of the scaled scores (-log2 sum 2^(s*scale*log2e))
 *   coef   [h][i]            fp32, signed branch weights (diff: [1, -lambda];
 *                            N-diff: [+l0, -l1, +l2, ...])
 *
 * Strides of a dta_tensor (dta_attn_fwd / dta_attn_bwd; tests/test_gpu_abi_layouts.py):
 *  - the innermost dimension (d, e) is contiguous: there is no stride for it;
 *  - ptr and every stride are multiples of 16 bytes (8 elements of a 16-bit dtype, 4 of fp32)
 *    and no stride is negative; anything else returns DTA_ERR_INVALID before any launch;
 *  - beyond that each tensor's sb, st, sh, si are free and independent of every other
 *    tensor's: head-major ([b][h][t]..), row-padded, branch-interleaved ([b][t][i][h][d]) and
 *    branch-outer ([b][i][t][h][d]) views all compute the same values, and no
 *    layout is refused.  An input may have a zero stride (one K / V for every batch row,
 *    sb = 0) or overlapping rows; an output's elements must not overlap;
 *  - speed: the 16-bit plans with head_size >= 32 stream K_i / V (and, in the key-major
 *    backward, Q_i / dO) tiles by LDS-DMA through 32-bit buffer descriptors when, for each of
 *    those tensors, every branch of a row lies inside the row's stride and the rows span less
 *    than 2 GiB:
 *        (n_terms - 1) * si + head_size <= st   (V, dO: dv <= st)   and   T * st * sizeof(dtype) < 2^31
 *    (csrc/layout_checks.h; n_terms: of the launch's branch group).  The packed projection
 *    layout, head-major and row-padded layouts satisfy it.  Other layouts (branch-outer Q / K,
 *    rows 2^25 elements apart) run the same kernels with the tiles staged through 64-bit
 *    addresses: same results -- bitwise, except that bf16 dQ without dropout takes its row
 *    constants in another rounding order -- at a lower speed.
 */
#ifndef DIFFATTN_H_
#define DIFFATTN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTA_ABI_VERSION 9   /* 9: dta_attn_extend (several new rows over the KV cache), dta_extend_supported;
                                  still 9, added without a bump (no existing struct or entry point changed):
                                  dta_attn_decode_ragged, dta_attn_extend_ragged (per-sequence lengths) -- the
                                  presence of the symbols is the capability check (dlsym / hasattr);
                                  still 9, added the same way: dta_attn_decode_paged, dta_attn_extend_paged
                                  (block-table KV cache over a pool of pages);
                                  still 9, added the same way: dta_attn_decode_paged_fp8, dta_kv_quant_rows
                                  (e4m3fn pages with per-(row, head) scales);
                                  still 9, added the same way: dta_kv_step_rows (a step's RoPE and cache
                                  scatter in one launch);
                                  still 9, added the same way: dta_sample_rows (seeded temperature /
                                  top-k / top-p sampling, one token per logits row);
                                  still 9, added the same way: dta_penalize_rows (sampling penalties, logit
                                  bias and min-p over logits rows), dta_penalize_rows_workspace_bytes;
                               8: lse_c workspace (the key-major kernel folds |c_i| into its probabilities);
                               7: per-stage backward branch-group caps (group_max_dq, group_max_dkdv);
                               6: obr_dtype (fp16 O_i for 16-bit activations);
                               5: RoPE of Q_i at the forward's load (rope_freqs, q_rot);
                               4: Obr is fp32 for every dtype; any n_terms >= 1 */

enum dta_dtype { DTA_BF16 = 0, DTA_F16 = 1, DTA_F32 = 2 };

enum dta_status {
  DTA_OK = 0,
  DTA_ERR_INVALID = -1,      /* bad shape / stride / pointer / argument   */
  DTA_ERR_UNSUPPORTED = -2,  /* head_size / n_terms / dtype not built     */
  DTA_ERR_LAUNCH = -3,       /* hipLaunch / hipMemsetAsync failed         */
  DTA_ERR_DROPOUT = -4       /* attention dropout p outside [0, 1)         */
};

typedef struct dta_tensor {
  void* ptr;
  int64_t sb, st, sh, si;    /* strides for [b][t][h][i]; si unused for V/O */
} dta_tensor;

/* Forward of the fused N-branch causal differential attention core.
 * Replaces, for all heads at once, DiffHead.forward's scores/mask/softmax/
 * dropout/combine/@V (diff_transformer.py:57-72), the per-head loop
 * (diff_transformer.py:89) and AlternatingDiffHead's branch loop
 * (Ndiff_transformer.py:102-125; RoPE: K_i beforehand by dta_rope, Q_i at load, rope_freqs).
 * O = sum_i coef[h][i] * softmax(mask(Q_i K_i^T / sqrt(hs))) V. */
typedef struct dta_attn_fwd_args {
  int32_t dtype;             /* enum dta_dtype */
  int32_t B, T, H, n_terms, head_size, dv;
  float scale;               /* 1/sqrt(head_size) (diff_transformer.py:57) */
  float dropout_p;           /* attention-map dropout in [0, 1) (diff_transformer.py:66-67):
                                element (q, k) of map i of head h, batch b is kept iff
                                fmix32((key + q*0x9e3779b1) ^ (k*0x7feb352d)) >= p*2^32,
                                key = fmix32(seed_lo ^ fmix32(((b*H + h)*N + i) + seed_hi))
                                (fmix32: murmur3's finaliser), kept elements x 1/(1-p);
                                the row sums normalising the map see every element */
  dta_tensor q, k, v;        /* inputs */
  dta_tensor o;              /* output, combined */
  dta_tensor obr;            /* output [i][b][t][h][e]: sb,st,sh,si = strides of b,t,h,i; fp32 or fp16 (obr_dtype) */
  float* lse;                /* output fp32 [i][b][h][t], contiguous */
  const float* coef;         /* fp32 [h][i], contiguous */
  uint64_t dropout_seed;     /* with dropout_p > 0: the mask's seed (pass the same to dta_attn_bwd) */
  /* ABI 5, optional: RoPE of Q_i fused into the load (Ndiff_transformer.py:104-109).
   * With rope_freqs (fp32 [T][head_size/2][2] (cos, sin), 16-byte aligned) q holds the
   * UN-rotated Q_i; the kernel rotates each row as it loads it and writes the rotated row
   * to q_rot (same shape as q, dtype) for dta_attn_bwd.  k must already be rotated
   * (dta_rope over the K_i only).  NULL: q is used as given. */
  const float* rope_freqs;
  dta_tensor q_rot;
  int32_t obr_dtype;         /* ABI 6: 0 / DTA_F32 = obr is fp32; DTA_F16 = fp16 (16-bit dtype only:
                                2^-11 resolution, eight times bf16's, half the bytes of fp32) */
} dta_attn_fwd_args;

int dta_attn_fwd(const dta_attn_fwd_args* a, void* stream);

/* Backward of dta_attn_fwd (the autograd of diff_transformer.py:57-72 and
 * Ndiff_transformer.py:102-125): dQ_i, dK_i, dV and d(coef).  Maps are
 * recomputed from LSE; nothing T x T is stored and no atomics touch dQ.
 * Two fused kernels: a query-major one (delta_i = <dO, O_i>, dQ_i, d(coef))
 * and a key-major one (dK_i, dV).  dcoef[h][i] = sum_{b,t} <dO, A_i V>
 * (SURVEY semantic 5), from which autograd reaches the lambda_q and lambda_k
 * params through get_lambda (diff_transformer.py:41-48).
 * Workspaces (caller-allocated, see dta_attn_bwd_workspace_bytes):
 *   delta   fp32 [i][b][h][t]: PRIVATE to the backward.  The DQ stage writes it in an
 *           encoding only the DKDV stage of the same call reads (row constants relative
 *           to each branch group's first branch, re-based in place where the two stages
 *           group branches differently).  Run DTA_BWD_DQ exactly once per backward and
 *           DTA_BWD_DKDV after it on the same delta; never read or reuse it otherwise.
 *           When the stages run as separate calls, both calls must pass the SAME
 *           group_max_dq and group_max_dkdv (the DQ stage encodes delta for the DKDV
 *           grouping those caps give; different caps in the DKDV call decode it wrongly).
 *   dq_f32  optional fp32 [b][t][h][i][d] contiguous: when dq.ptr is NULL the
 *           dQ kernel writes fp32 here instead (callers that post-process dQ,
 *           e.g. the inverse RoPE, keep full precision). */
typedef struct dta_attn_bwd_args {
  int32_t dtype;
  int32_t B, T, H, n_terms, head_size, dv;
  float scale;
  float dropout_p;           /* as dta_attn_fwd_args; obr must be the forward's (dropped) O_i */
  dta_tensor q, k, v, obr;
  const float* lse;          /* fp32 [i][b][h][t] from the forward */
  const float* coef;         /* fp32 [h][i] */
  dta_tensor dout;           /* dO [b][t][h][e] */
  dta_tensor dq, dk, dv_out; /* outputs (dtype) */
  float* dcoef;              /* output fp32 [h][i] (overwritten; all zero when B * T == 0, written by
                                the DQ stage, or by PRE without dcoef_partial) */
  float* delta;              /* workspace fp32 [i][b][h][t] */
  float* dq_f32;             /* see above */
  int32_t stages;            /* 0 = all; else bitmask of DTA_BWD_PRE (zero dcoef; a no-op when
                                dcoef_partial is given, whose ordered reduce writes dcoef whole),
                                DTA_BWD_DQ (query-major kernel), DTA_BWD_DKDV
                                (key-major kernel) -- lets a caller bracket one
                                kernel with events on the same stream; DQ must
                                run before DKDV (it produces delta) */
  const float* rope_freqs;   /* optional fp32 [T][head_size/2][2] (cos, sin) table,
                                16-byte aligned: q and k are the RoPE'd Q_i / K_i
                                (Ndiff_transformer.py:104-109), and dQ / dK are
                                returned w.r.t. the UN-rotated projections -- the
                                inverse rotation (apply_rotary_emb's backward) runs
                                in the kernels' epilogues, no extra pass or buffer */
  float* dcoef_partial;      /* optional fp32 workspace, dta_attn_bwd_dcoef_partial_bytes:
                                with it dcoef is summed from per-wave partials in a fixed
                                order (bitwise reproducible run to run); without it the
                                query-major kernel adds into dcoef by float atomics */
  uint64_t dropout_seed;     /* the forward's dropout seed */
  int32_t obr_dtype;         /* ABI 6: as dta_attn_fwd_args (the forward's obr) */
  int32_t group_max_dq;      /* ABI 7, optional (0 = the library's default per stage): the largest
                                branch group the DQ stage runs as one launch (n_terms above it run
                                as groups of the largest built branch count <= this cap, one launch
                                each).  Defaults: 4 for fp32; 16-bit: 2 at head_size 128 and at 64
                                with n_terms >= 4, else 4.  Setting it to 4 forces every built
                                native plan (the GPU tests check each one). */
  int32_t group_max_dkdv;    /* ABI 7, as group_max_dq for the DKDV stage.  Defaults: 4 for fp32;
                                16-bit: 2 at head_size >= 64, else 4.  Groups after the first
                                add their dV into the first group's. */
  float* dv_f32;             /* ABI 7, optional fp32 workspace [b][t][h][e] contiguous (B*T*H*dv
                                floats, 16-byte aligned): where the DKDV stage runs more than one
                                group (dta_attn_bwd_dkdv_groups > 1), the running dV sum stays here
                                in fp32 and only the last group rounds it to dtype.  NULL: each later
                                group adds into dv_out (one extra 16-bit rounding per group). */
  float* lse_c;              /* ABI 8, optional fp32 workspace [i][b][h][t] (n_terms*B*H*T floats, 16-byte
                                aligned), PRIVATE to the backward like delta: with 16-bit activations and
                                no dropout the DQ stage writes each row's stored LSE_i + log2|c_i| here and
                                the DKDV stage seeds its scores with it, so its probabilities come out
                                already scaled by |c_i| (one VALU op per element less in dV's operand).
                                When the stages run as separate calls, the DQ and the DKDV call must pass
                                the SAME lse_c (both the buffer or both NULL): the DKDV stage reads what
                                the DQ stage wrote there, and with NULL in either it takes the other path.
                                Range: the kernel packs |c_i| P and |c_i| P (dP - delta_i) to dtype.  bf16
                                has fp32's exponent range: |c_i| < 2^64.  fp16 overflows at 65504 and its
                                absolute step below 2^-14 is 2^-24, so |c_i| max|P (dP - delta_i)| must stay
                                below 65504 and a branch whose |c_i| P (dP - delta_i) lies under ~1e-4
                                loses bits; 1e-3 <= |c_i| <= 1e3 on unit-variance activations is measured
                                (profiles/coef_scale_errors.json: every branch's dQ_i / dK_i error equals
                                the unfolded path's, independent of |c_i|).  Outside that range pass NULL.
                                NULL (or fp32 / dropout): the unfolded kernels. */
} dta_attn_bwd_args;

enum { DTA_BWD_PRE = 1, DTA_BWD_DQ = 2, DTA_BWD_DKDV = 4 };

int dta_attn_bwd(const dta_attn_bwd_args* a, void* stream);
size_t dta_attn_bwd_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t n_terms,
                                    int32_t head_size);
size_t dta_attn_bwd_dcoef_partial_bytes(int32_t B, int32_t T, int32_t H, int32_t n_terms);
/* The number of dK/dV launches (branch groups) dta_attn_bwd runs for this shape with the given
 * group_max_dkdv (0 = default); 0 if the shape is unsupported or the cap is negative (which
 * dta_attn_bwd rejects).  > 1: pass dv_f32. */
int dta_attn_bwd_dkdv_groups(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t group_max_dkdv);

/* Cross-head LayerNorm x out_scale (GroupLayerNorm.forward,
 * diff_transformer.py:15-20, then `out * (1 - self.lambda_init)`,
 * diff_transformer.py:90-91; same at Ndiff_transformer.py:33-38,145-146).
 * Rows of width C; y = ((x - mean) * rstd * w + b) * out_scale.
 * mean/rstd (fp32 [rows]) are saved for dta_ln_bwd. */
typedef struct dta_ln_args {
  int32_t dtype;
  int64_t rows, C;
  float eps, out_scale;
  const void* x; int64_t x_stride;   /* row stride, elements */
  void* y; int64_t y_stride;
  const float* w; const float* b;    /* fp32 [C] */
  float* mean; float* rstd;          /* fp32 [rows] */
  /* backward only */
  const void* dy; int64_t dy_stride;
  void* dx; int64_t dx_stride;
  float* dw; float* db;              /* fp32 [C], accumulated (caller zeroes) */
  float* partial;                    /* optional fp32 workspace (dta_ln_bwd_workspace_bytes):
                                        per-block column partials summed in a fixed order, so
                                        dw/db are bitwise reproducible; 16-byte aligned;
                                        NULL: float atomics */
  int32_t io_dtype;                  /* 0: y / dy have `dtype`; else 1 + the y / dy dtype code,
                                        with dtype = DTA_F32 and y / dy DTA_BF16 or DTA_F16 (an fp32
                                        residual stream normalised straight into the autocast
                                        dtype, and its backward from that dtype's gradient) */
  /* residual fusion, io_dtype != 0 only (NULL = off): the pre-LN residual add of a
   * Block (diff_transformer.py:121-125, x + attn(ln1(x)) feeding ln2) in the same pass */
  const void* res; int64_t res_stride;   /* fwd: normalises x + res (res in the y dtype) ... */
  float* xo; int64_t xo_stride;          /* ... and writes x + res here (fp32, required with res) */
  const float* dres; int64_t dres_stride;  /* bwd: dx += dres (fp32 gradient of the residual branch) */
  void* dx16; int64_t dx16_stride;       /* bwd: dx also written in the y dtype */
} dta_ln_args;

int dta_ln_fwd(const dta_ln_args* a, void* stream);
int dta_ln_bwd(const dta_ln_args* a, void* stream);
size_t dta_ln_bwd_workspace_bytes(int64_t rows, int64_t C);

/* Interleaved-pair RoPE of every Q_i and K_i (apply_rotary_emb,
 * Ndiff_transformer.py:11-22 / control.py:11-22, rotation in fp32 then cast).
 * inverse != 0 applies the conjugate rotation (its backward).
 * src may be fp32 (src_f32 != 0) or dtype; dst is dtype.
 * freqs: fp32 [T][head_size/2][2] = view_as_real(freqs_cis[:T]). */
typedef struct dta_rope_args {
  int32_t dtype;
  int32_t B, T, H, n_terms, head_size;
  int32_t inverse, src_f32;
  dta_tensor src, dst;               /* [b][t][h][i][d] */
  const float* freqs;
} dta_rope_args;

int dta_rope(const dta_rope_args* a, void* stream);

/* One-token decode over a KV cache (incremental generate).
 * Replaces, for the newest position only, the full-prefix recompute that
 * generate() does per token (diff_transformer.py:177-185; the same loop in
 * Ndiff_transformer.py and control.py:163-171): for every (b, h)
 *   o = sum_i coef[h][i] * softmax(q_i . K_i[0:length]^T * scale) V[0:length]
 * which is the last row of dta_attn_fwd's output at T = length (the newest key
 * is the query's own position, so the causal mask keeps every cached key).
 * q: [b][.][h][i][d] (st ignored), k_cache [b][t][h][i][d], v_cache [b][t][h][e],
 * o [b][.][h][e] (st ignored).  head_size % 8 == 0, head_size <= 128,
 * n_terms <= 4, dv <= 256; every tensor 16-byte aligned with strides that are
 * multiples of 16 bytes.  workspace: fp32, dta_attn_decode_workspace_bytes
 * (covers both plans).  Plans: a split-key plan -- key chunks scored by separate
 * workgroups, then one combine launch -- for (head_size, dv) in {(32,64),
 * (64,128), (128,256)} and, with n_terms = 1, dv = head_size in {64, 128}; a
 * single-pass workgroup per (b, h) otherwise.  The split plan uses 256-key
 * chunks, or 512-key chunks when ceil(t_cap/256) * H * B >= 8192 workgroups;
 * the choice depends on t_cap only, so calls with the same t_cap reduce in the
 * same order whatever their length.  It is used while ceil(t_cap/chunk) *
 * n_terms <= 2048 (the combine's LDS weights). */
typedef struct dta_attn_decode_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;            /* valid cached keys, including the new token's */
  int32_t t_cap;             /* workspace row length (>= length) */
  float scale;
  dta_tensor q, k_cache, v_cache, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* length_dev; /* optional device int32: the valid length, read by the
                                kernels (graph replay with a moving position); then
                                `length` is only its upper bound and sizes the grid.
                                Precondition 1 <= *length_dev <= length <= t_cap; the
                                kernels clamp it to [0, length] */
} dta_attn_decode_args;
int dta_attn_decode(const dta_attn_decode_args* a, void* stream);
size_t dta_attn_decode_workspace_bytes(int32_t B, int32_t H, int32_t n_terms, int32_t head_size, int32_t dv,
                                       int32_t t_cap);

/* dta_attn_decode for a ragged batch: every sequence of the batch at its own length.
 * Replaces the same reference lines as dta_attn_decode (the per-token full-prefix
 * recompute of generate(), diff_transformer.py:177-185; Ndiff_transformer.py generate;
 * control.py:163-171) for B sequences whose prompts, accepted tokens or restarts left
 * them at different positions: for every (b, h)
 *   o[b] = sum_i coef[h][i] * softmax(q_i[b] . K_i[b][0:len_b]^T * scale) V[b][0:len_b]
 * with len_b = lengths_dev[b], the number of valid cached keys of sequence b (its new
 * token's own row included).  Everything else -- tensors, alignment, plans, workspace
 * (dta_attn_decode_workspace_bytes), the chunk choice from t_cap only -- is
 * dta_attn_decode's; `length` is the host upper bound of every len_b and sizes the
 * grid (t_cap needs no host knowledge of the lengths).  Every kernel clamps len_b to
 * [0, length].  len_b == 0 writes zeros (no NaN, no Inf).  Cache rows >= len_b of
 * sequence b may hold anything, NaN included: they never reach the output, and a key
 * chunk wholly past len_b exits before it touches memory, so the cache traffic of a
 * call is sum_b len_b rows, not B * max.  With every len_b = L the output is bitwise
 * equal to dta_attn_decode at length = L (same t_cap).  lengths_dev NULL or not
 * 4-byte aligned: DTA_ERR_INVALID. */
typedef struct dta_attn_decode_ragged_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;            /* host upper bound of every lengths_dev[b] (<= t_cap); sizes the grid */
  int32_t t_cap;             /* workspace row length (>= length) */
  float scale;
  dta_tensor q, k_cache, v_cache, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* lengths_dev;/* device int32 [B], required: valid cached keys of sequence b */
} dta_attn_decode_ragged_args;
int dta_attn_decode_ragged(const dta_attn_decode_ragged_args* a, void* stream);

/* Several new rows over a KV cache (ABI 9): append to a live cache, scoring of
 * candidate tokens, chunked prefill.  Replaces DiffHead.forward's scores / mask /
 * softmax / combine / @V (diff_transformer.py:57-72; Ndiff_transformer.py:102-125)
 * for the Tq NEWEST rows of the window only: query row r sits at absolute position
 * pos + r and for every (b, h)
 *   o[b][r][h] = sum_i coef[h][i] * softmax_j(q_i[b][r][h] . K_i[b][j][h] * scale, j <= pos + r) V[b][j][h]
 * which is rows pos .. pos+Tq-1 of dta_attn_fwd's output at T = pos + Tq, and with
 * Tq = 1 dta_attn_decode at length = pos + 1.  Inference only: nothing but o is
 * written (no Obr, no LSE, no dropout, no workspace).
 * Mask: key j is kept for row r iff j <= pos + r (absolute positions; pos need
 * not be a multiple of any tile size).  Cache rows 0 .. pos+Tq-1 must be valid --
 * the new rows' own K_i / V are written by the caller first; rows pos+Tq .. t_cap-1
 * may hold anything, NaN included: they are never multiplied into the result.
 * q [b][t < Tq][h][i][d] (rotated already for RoPE models), k_cache [b][t][h][i][d],
 * v_cache [b][t][h][e] (strided views of the packed cache buffer, as for decode),
 * o [b][t < Tq][h][e].  head_size % 16 == 0, 16 <= head_size <= 128; dv % 32 == 0,
 * dv <= 256; 1 <= n_terms <= 8; every dtype; every tensor 16-byte aligned with
 * strides that are multiples of 16 bytes; anything else is DTA_ERR_UNSUPPORTED
 * (dta_extend_supported tells beforehand).  Tq == 0 or B*H == 0: DTA_OK, no launch.
 * pos < 0, pos + Tq > t_cap, a null pointer or a misaligned stride: DTA_ERR_INVALID. */
typedef struct dta_attn_extend_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* new query rows */
  int32_t pos;               /* absolute position of query row 0; keys 0 .. pos+Tq-1 are valid */
  int32_t t_cap;             /* rows of the cache views (>= pos + Tq) */
  float scale;
  dta_tensor q, k_cache, v_cache, o;
  const float* coef;         /* fp32 [h][i] */
} dta_attn_extend_args;
int dta_attn_extend(const dta_attn_extend_args* a, void* stream);
int dta_extend_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv);

/* dta_attn_extend for a ragged batch (same reference lines: diff_transformer.py:57-72,
 * Ndiff_transformer.py:102-125, for the newest rows only): sequence b appends count_b
 * real rows at its own position pos_b -- the verification of speculated tokens (each
 * sequence accepted a different number before), a second turn of different lengths, a
 * fresh sequence (pos_b = 0) joining a live batch.  q and o hold Tq rows per sequence,
 * padded; for row r of sequence b
 *   r <  count_b:  o[b][r][h] = sum_i coef[h][i] * softmax_j(q_i[b][r][h] . K_i[b][j][h] * scale, j <= pos_b + r) V[b][j][h]
 *                  (dta_attn_extend's formula with pos = pos_b)
 *   r >= count_b:  o[b][r][h] = 0 (q rows count_b .. Tq-1 are never read)
 * pos_dev: device int32 [B], required; count_dev: device int32 [B], or NULL = Tq for
 * every sequence.  The kernel clamps pos_b to [0, t_cap - Tq] and count_b to [0, Tq],
 * so no device value can index past the views.  Valid cache rows of sequence b are
 * 0 .. pos_b + count_b - 1 (the caller writes the new rows' K_i / V first); every row
 * above may hold anything, NaN included: it is never multiplied into the result.  A
 * workgroup reads key tiles up to its own sequence's last needed one only, and a query
 * tile without a real row writes its zeros and exits; count_b == 0 divides nothing.
 * Shapes, alignment, plans and dta_extend_supported are dta_attn_extend's; with every
 * pos_b = pos and count_dev NULL the output is bitwise equal to dta_attn_extend's.
 * Tq > t_cap, a null pos_dev, a pointer not 4-byte aligned, a null tensor or a
 * misaligned stride: DTA_ERR_INVALID.  Tq == 0 or B*H == 0: DTA_OK, no launch. */
typedef struct dta_attn_extend_ragged_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded) */
  int32_t t_cap;             /* rows of the cache views (>= Tq) */
  float scale;
  dta_tensor q, k_cache, v_cache, o;
  const float* coef;         /* fp32 [h][i] */
  const int32_t* pos_dev;    /* device int32 [B]: absolute position of query row 0 of sequence b */
  const int32_t* count_dev;  /* device int32 [B] or NULL: real new rows of sequence b */
} dta_attn_extend_ragged_args;
int dta_attn_extend_ragged(const dta_attn_extend_ragged_args* a, void* stream);

/* Paged KV cache: dta_attn_decode_ragged / dta_attn_extend_ragged with the cache rows
 * reached through a per-sequence block table into a shared pool of fixed-size pages, so
 * a batch holds sum_b ceil(len_b / P) pages instead of B * t_cap rows, a finished
 * sequence's pages go to a new one, and sequences with a common prefix share its pages.
 * Replaces the same reference lines (the per-token full-prefix recompute of generate(),
 * diff_transformer.py:177-185; Ndiff_transformer.py generate; control.py:163-171, and
 * diff_transformer.py:57-72 for the newest rows).
 *   k_pool [page][row < P][h][i][d]   sb = page stride, st = row stride
 *   v_pool [page][row < P][h][e]
 *   block_table_dev  device int32 [B][max_pages], contiguous
 * Key row j of sequence b is pool[block_table_dev[b][j / P]][j % P]:
 *   decode:  o[b] = sum_i coef[h][i] * softmax(q_i[b] . K_i(b, 0:len_b)^T * scale) V(b, 0:len_b)
 *   extend:  dta_attn_extend_ragged's formula with K_i[b][j] = K_i(b, j), V[b][j] = V(b, j)
 * page_size P is 32, 64, 128 or 256 (the multiples of the extend kernel's 32-key tile
 * that divide the decode chunk: a decode chunk is a whole number of pages and a key tile
 * never straddles a page); t_cap, the logical capacity of a sequence, must equal
 * max_pages * page_size and plays t_cap's part in the ragged calls (workspace size
 * dta_attn_decode_workspace_bytes(.., t_cap), chunk choice, the clamp of pos_b to
 * [0, t_cap - Tq]); n_pages is the number of pages the pool views hold.
 * Table entries: only entries p < ceil(len_b / P) of row b are read (extend:
 * p < ceil((pos_b + count_b) / P)); the rest may hold anything.  Every id that is read is
 * clamped to [0, n_pages - 1] before it forms an address, as len_b, pos_b and count_b are
 * clamped, so no device value can index outside the pool.  Rows >= len_b inside a used
 * page, and every page no used entry names, may hold anything, NaN included.  A decode
 * chunk wholly past len_b exits before it touches memory; len_b == 0 writes zeros; extend
 * writes zeros to rows count_b .. Tq-1 and a query tile without a real row exits.
 * Bitwise relation: the kernels do the ragged kernels' operations in the same order, only
 * the addresses differ.  Cut a contiguous cache (B, max_pages * P, ..) into pages, place
 * them anywhere in a pool and describe them by a block table: the outputs equal
 * dta_attn_decode_ragged / dta_attn_extend_ragged on the contiguous cache bit for bit, at
 * the same t_cap.
 * Errors: everything the ragged entry points reject, and DTA_ERR_INVALID for a null or
 * not 4-byte aligned block_table_dev, a page_size outside {32, 64, 128, 256},
 * n_pages < 1, max_pages < 1 or t_cap != max_pages * page_size.  dta_extend_supported is
 * the capability check of the extend call. */
typedef struct dta_attn_decode_paged_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;            /* host upper bound of every lengths_dev[b] (<= t_cap); sizes the grid */
  int32_t t_cap;             /* = max_pages * page_size; workspace row length */
  float scale;
  dta_tensor q, k_pool, v_pool, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* lengths_dev;/* device int32 [B], required: valid cached keys of sequence b */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
} dta_attn_decode_paged_args;
int dta_attn_decode_paged(const dta_attn_decode_paged_args* a, void* stream);

typedef struct dta_attn_extend_paged_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded) */
  int32_t t_cap;             /* = max_pages * page_size (>= Tq) */
  float scale;
  dta_tensor q, k_pool, v_pool, o;
  const float* coef;         /* fp32 [h][i] */
  const int32_t* pos_dev;    /* device int32 [B]: absolute position of query row 0 of sequence b */
  const int32_t* count_dev;  /* device int32 [B] or NULL: real new rows of sequence b */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
} dta_attn_extend_paged_args;
int dta_attn_extend_paged(const dta_attn_extend_paged_args* a, void* stream);

/* FP8 paged KV cache (still ABI 9; the presence of the two symbols is the capability
 * check): the page pool holds one byte per element and a decode step reads
 * N*hs + dv + 4*(N+1) bytes per (row, head) instead of 2*(N*hs + dv).
 * Format:
 *   elements  OCP e4m3fn (gfx950's native fp8, torch.float8_e4m3fn; not fnuz)
 *   scales    fp32, one per (cache row, head, branch i) for K_i and one per (cache row,
 *             head) for V: scale_pool [page][row < P][h][N+1], contiguous inside a page,
 *             index N holding V's scale; scale_page_stride (floats) >= P * H * (N+1)
 *   k_pool / v_pool   today's row layout [K (H, N, hs) | V (H, dv)], one byte per element,
 *             described by dta_tensor with strides in elements = bytes
 *   quantisation of one vector x (a K_i head row of hs values, a V head row of dv values):
 *             amax = max|x| (fp32, of the values as the activation dtype stores them),
 *             scale = amax / 448, byte = e4m3_rne(clamp(x / scale, -448, 448)); the clamp is
 *             explicit and precedes the conversion; amax == 0 gives scale 0 and bytes 0 with
 *             no division; non-finite input is undefined, as in the 16-bit cache
 *   dequantisation    x^ = float(byte) * scale, never materialised in memory
 *
 * dta_attn_decode_paged_fp8 replaces the lines dta_attn_decode_paged does (the per-token
 * full-prefix recompute of generate(), diff_transformer.py:177-185; Ndiff_transformer.py
 * generate; control.py:163-171) on such a pool:
 *   o[b] = sum_i coef[h][i] * softmax(q_i[b] . K^_i(b, 0:len_b)^T * scale) V^(b, 0:len_b)
 * dtype is the dtype of q and o.  The dot product of a K row is multiplied by its scale
 * once per (row, branch); V's scale is folded into the probability before the V
 * accumulation and the row sum uses the unscaled probability; all sums are fp32.  Plans,
 * chunk choice from t_cap, workspace (dta_attn_decode_workspace_bytes), the clamps of
 * len_b and of every page id, the early exit of a chunk past len_b (before any load, scale
 * loads included) and zeros for len_b == 0 are dta_attn_decode_paged's.  Rows >= len_b and
 * unowned pages may hold any bytes and any scales, NaN and Inf included.
 * Errors: everything dta_attn_decode_paged rejects (the pool views are checked as byte
 * views), and DTA_ERR_INVALID for a null or not 4-byte aligned scale_pool_dev, a
 * scale_page_stride below P * H * (N+1), or a byte-pool row or page stride that is not a
 * multiple of 16. */
typedef struct dta_attn_decode_paged_fp8_args {
  int32_t dtype;             /* of q and o */
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;            /* host upper bound of every lengths_dev[b] (<= t_cap); sizes the grid */
  int32_t t_cap;             /* = max_pages * page_size; workspace row length */
  float scale;
  dta_tensor q, k_pool, v_pool, o;   /* k_pool / v_pool: e4m3fn bytes, strides in bytes */
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* lengths_dev;/* device int32 [B], required: valid cached keys of sequence b */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
  const float* scale_pool_dev;     /* fp32 [page][row < P][h][N+1] */
  int64_t scale_page_stride;       /* floats from one page's scales to the next */
} dta_attn_decode_paged_fp8_args;
int dta_attn_decode_paged_fp8(const dta_attn_decode_paged_fp8_args* a, void* stream);

/* The write side: quantise a step's new rows into the pool.  Replaces, for an fp8 pool,
 * the scatter of the new K_i / V rows into the cache (the index_put_ of
 * kv_cache._paged_attention_step; in the reference those rows are recomputed per token,
 * diff_transformer.py:177-185).  k_new [b][t < Tn][h][i][d] and v_new [b][t < Tn][h][e] are
 * strided views in the activation dtype (16-byte aligned, strides multiples of 16 bytes;
 * K may be the RoPE temporary, V a slice of the packed projection).  slot_dev: device int32
 * [B * Tn], slot = page * page_size + row of row (b, t); padding rows point into the spare
 * page, page n_pages: the pool views and the scale pool hold n_pages + 1 pages.  Every slot
 * is clamped to [0, (n_pages + 1) * page_size - 1] before it forms an address.  Writes the
 * bytes and the N+1 scales of every (row, head) in the format above and nothing else.
 * DTA_ERR_UNSUPPORTED: head_size or dv not a multiple of 16 (or above 128 / 256), n_terms
 * outside 1..4.  DTA_ERR_INVALID: a page_size outside {32, 64, 128, 256}, n_pages < 1, a
 * null or misaligned pointer or stride, a scale_page_stride below P * H * (N+1).
 * B * Tn == 0: DTA_OK, no launch. */
typedef struct dta_kv_quant_rows_args {
  int32_t dtype;             /* of k_new and v_new */
  int32_t B, Tn, H, n_terms, head_size, dv;
  int32_t page_size, n_pages;
  dta_tensor k_new, v_new;
  dta_tensor k_pool, v_pool; /* e4m3fn bytes, strides in bytes, n_pages + 1 pages */
  float* scale_pool_dev;     /* fp32 [page][row < P][h][N+1], n_pages + 1 pages */
  int64_t scale_page_stride;
  const int32_t* slot_dev;   /* device int32 [B * Tn] */
} dta_kv_quant_rows_args;
int dta_kv_quant_rows(const dta_kv_quant_rows_args* a, void* stream);

/* The multi-row step on an fp8 pool (still ABI 9; the presence of the two symbols is the
 * capability check): dta_attn_extend_paged with the cache rows read as e4m3fn bytes and
 * scales in the format above, one launch for what would otherwise be count_b
 * dta_attn_decode_paged_fp8 launches per sequence (append to a cached conversation,
 * verification of draft tokens, scoring; replaces the same reference lines as
 * dta_attn_extend_paged, diff_transformer.py:57-72 for the newest rows).  For row r of
 * sequence b
 *   r <  count_b:  o[b][r][h] = sum_i coef[h][i] * softmax_j(q_i[b][r][h] . K^_i(b, j)[h] * scale, j <= pos_b + r) V^(b, j)[h]
 *   r >= count_b:  o[b][r][h] = 0
 * with K^_i(b, j), V^(b, j) the dequantised row j of sequence b (x^ = float(byte) * scale),
 * never materialised in memory.  dtype is the dtype of q, o and both MFMA operands.
 * Arithmetic:
 *   K  the K_i image of a key tile holds the bare byte values (every e4m3 value is exact in
 *      bf16, f16 and f32); the fp32 accumulator of q_i . byte(K_i[j]) is multiplied by
 *      k_scale[j][h][i] once per (key, branch), as in dta_attn_decode_paged_fp8
 *   V  the V image holds V^ = float(byte) * v_scale[j][h] rounded once to the operand type
 *      (exact in f32).  V's scale is not folded into the probability: P is packed to the
 *      operand type for the P V product, and an f16 probability times amax / 448 underflows
 * Everything else is dta_attn_extend_paged's: the two passes, no workspace, only o written,
 * the clamps of pos_b to [0, t_cap - Tq], of count_b to [0, Tq] and of every page id to
 * [0, n_pages - 1], the table entries read (p < ceil((pos_b + count_b) / P)), zeros for
 * rows count_b .. Tq-1, and the exit of a query tile without a real row before any load.
 * Rows >= pos_b + count_b inside a used page are staged as zeros and their scales are never
 * loaded; those rows and every page no used entry names may hold any bytes and any scales,
 * NaN and Inf included.
 * dta_extend_fp8_supported: 1 for the shapes both dta_extend_supported and
 * dta_kv_quant_rows take (head_size a multiple of 16 up to 128, dv a multiple of 32 up to
 * 256, n_terms 1..4, dtype bf16 / f16 / f32), else 0.
 * Errors: everything dta_attn_extend_paged rejects (the pool views are checked as byte
 * views), and DTA_ERR_INVALID for a null or not 4-byte aligned scale_pool_dev, a
 * scale_page_stride below P * H * (N+1), or a byte-pool row or page stride that is not a
 * multiple of 16; DTA_ERR_UNSUPPORTED where dta_extend_fp8_supported is 0.  Tq == 0 or
 * B*H == 0: DTA_OK, no launch. */
typedef struct dta_attn_extend_paged_fp8_args {
  int32_t dtype;             /* of q and o */
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded) */
  int32_t t_cap;             /* = max_pages * page_size (>= Tq) */
  float scale;
  dta_tensor q, k_pool, v_pool, o;   /* k_pool / v_pool: e4m3fn bytes, strides in bytes */
  const float* coef;         /* fp32 [h][i] */
  const int32_t* pos_dev;    /* device int32 [B]: absolute position of query row 0 of sequence b */
  const int32_t* count_dev;  /* device int32 [B] or NULL: real new rows of sequence b */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
  const float* scale_pool_dev;     /* fp32 [page][row < P][h][N+1] */
  int64_t scale_page_stride;       /* floats from one page's scales to the next */
} dta_attn_extend_paged_fp8_args;
int dta_attn_extend_paged_fp8(const dta_attn_extend_paged_fp8_args* a, void* stream);
int dta_extend_fp8_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv);

/* A short multi-row step on the split-key decode plan (still ABI 9; the presence of the
 * symbols is the capability check): 1 <= Tq <= 8 new rows per sequence -- the verification
 * of a short draft, the scoring of a few candidate tokens -- in one split launch and one
 * combine launch that load every cached K_i / V row once for all rows, where Tq
 * dta_attn_decode_ragged launches each re-read the cache and dta_attn_extend_ragged fills
 * ceil(Tq/32) * H * B workgroups only.  Replaces the same reference lines as the extend
 * entries (DiffHead.forward's scores / mask / softmax / combine / @V,
 * diff_transformer.py:57-72; Ndiff_transformer.py:102-125, for the newest rows only).
 * For row r of sequence b, with pos_b = pos_dev[b] and count_b = count_dev[b] (NULL: Tq)
 *   r <  count_b:  o[b][r][h] = sum_i coef[h][i] * softmax_j(q_i[b][r][h] . K_i[b][j][h] * scale, j <= pos_b + r) V[b][j][h]
 *   r >= count_b:  o[b][r][h] = 0 (q rows count_b .. Tq-1 are never read)
 * q [b][t < Tq][h][i][d], o [b][t < Tq][h][e], the caches as dta_attn_decode_ragged's
 * (dta_attn_decode_rows), dta_attn_decode_paged's (_paged) or dta_attn_decode_paged_fp8's
 * (_paged_fp8, same format and scale placement).  The new rows' own K_i / V are written
 * first; valid rows of sequence b are 0 .. pos_b + count_b - 1 and nothing above them is
 * loaded: not K, not V, not a scale, not a page id (entries p >= ceil((pos_b + count_b) /
 * P)); they may hold anything, NaN included.  count_b == 0 loads nothing at all.
 * Bitwise relation: every real row equals dta_attn_decode_ragged / _paged / _paged_fp8 at
 * lengths_dev[b] = pos_b + r + 1 on the same cache at the same t_cap, bit for bit: the chunk
 * choice from t_cap only, the split of a K row over lanes, the key a thread owns in the
 * softmax, the V row groups and every order of summation are the one-row kernels'.
 * Plans: the split-key shapes only -- (head_size, dv) in {(32,64), (64,128), (128,256)} with
 * n_terms 1..4, and n_terms = 1 with dv = head_size in {64, 128} -- every dtype, 16-/32-bit
 * or e4m3 cache, while ceil(t_cap/chunk) * n_terms <= 2048.  There is no single-pass plan:
 * anything else is DTA_ERR_UNSUPPORTED (dta_decode_rows_supported tells beforehand) and the
 * caller keeps its per-row or extend path.
 * workspace: fp32, dta_attn_decode_rows_workspace_bytes(.., t_cap, Tq) -- the one-row
 * split plan's partials and (max, sum) pairs times Tq.
 * The kernels clamp pos_b to [0, t_cap - Tq], count_b to [0, Tq] and every page id to
 * [0, n_pages - 1], so no device value can index outside cache, pool, workspace or LDS.
 * Errors: everything the matching decode / extend entry rejects (null or misaligned
 * pointers and strides, null pos_dev, t_cap < Tq, the paged and fp8 arguments), and
 * DTA_ERR_INVALID for Tq outside 1..8.  B*H == 0: DTA_OK, no launch. */
typedef struct dta_attn_decode_rows_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded), 1 .. 8 */
  int32_t t_cap;             /* rows of the cache views (>= Tq); sizes the grid and the workspace */
  float scale;
  dta_tensor q, k_cache, v_cache, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* pos_dev;    /* device int32 [B], required: absolute position of query row 0 of sequence b */
  const int32_t* count_dev;  /* device int32 [B] or NULL: real new rows of sequence b */
} dta_attn_decode_rows_args;
int dta_attn_decode_rows(const dta_attn_decode_rows_args* a, void* stream);
size_t dta_attn_decode_rows_workspace_bytes(int32_t B, int32_t H, int32_t n_terms, int32_t head_size, int32_t dv,
                                            int32_t t_cap, int32_t Tq);
int dta_decode_rows_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t Tq,
                              int32_t fp8_cache);

typedef struct dta_attn_decode_rows_paged_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded), 1 .. 8 */
  int32_t t_cap;             /* = max_pages * page_size (>= Tq) */
  float scale;
  dta_tensor q, k_pool, v_pool, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* pos_dev;    /* device int32 [B], required */
  const int32_t* count_dev;  /* device int32 [B] or NULL */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
} dta_attn_decode_rows_paged_args;
int dta_attn_decode_rows_paged(const dta_attn_decode_rows_paged_args* a, void* stream);

typedef struct dta_attn_decode_rows_paged_fp8_args {
  int32_t dtype;             /* of q and o */
  int32_t B, H, n_terms, head_size, dv;
  int32_t Tq;                /* query rows per sequence (padded), 1 .. 8 */
  int32_t t_cap;             /* = max_pages * page_size (>= Tq) */
  float scale;
  dta_tensor q, k_pool, v_pool, o;   /* k_pool / v_pool: e4m3fn bytes, strides in bytes */
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* pos_dev;    /* device int32 [B], required */
  const int32_t* count_dev;  /* device int32 [B] or NULL */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
  const float* scale_pool_dev;     /* fp32 [page][row < P][h][N+1] */
  int64_t scale_page_stride;       /* floats from one page's scales to the next */
} dta_attn_decode_rows_paged_fp8_args;
int dta_attn_decode_rows_paged_fp8(const dta_attn_decode_rows_paged_fp8_args* a, void* stream);

/* Shared-prefix decode on the paged cache (still ABI 9; the presence of the symbols is the
 * capability check): dta_attn_decode_paged / dta_attn_decode_paged_fp8 for a batch in which
 * groups of sequences have the same pool pages under their first rows -- the samples of one
 * prompt after a fork.  Same formula, same reference lines (the per-token full-prefix
 * recompute of generate(), diff_transformer.py:177-185; Ndiff_transformer.py generate;
 * control.py:163-171); what changes is that the shared rows are read from memory once per
 * group instead of once per member.
 * The plan, on the device:
 *   n_groups            G >= 0
 *   group_members_dev   int32 [G][8]: batch indices of the 2 .. 8 members of a group; -1 (any
 *                       value outside [0, B)) is an empty slot; a sequence is in at most one group
 *   group_rows_dev      int32 [G]: cache rows 0 .. rows-1 are the same pool pages in every
 *                       member's block-table row
 * A sequence in no group is handled exactly as by dta_attn_decode_paged.
 * Launches, in stream order, on the one-row workspace (dta_attn_decode_workspace_bytes):
 *   1. group pass, grid (chunks, H, G): a workgroup runs only for a chunk wholly below
 *      covered_g = floor(min(rows_g, min over members of len_b) / chunk) * chunk, looks the
 *      chunk's pages up in the first member's table, loads every K_i / V row, scale and page
 *      id once and writes each member's partial into that member's own one-row slot
 *   2. the one-row split launch, whose workgroups return before they touch the cache where
 *      their chunk lies below their sequence's covered rows
 *   3. the one-row combine, unchanged
 * Bitwise relation: the chunk is chosen as the one-row launch chooses it (from t_cap, H and
 * the whole B), and the lane split of a K row, the key a thread owns, the V row groups, every
 * order of summation and the fp8 scale placement are the one-row kernels'.  Given that the
 * shared rows are the same pages in every member's table, the output equals
 * dta_attn_decode_paged / dta_attn_decode_paged_fp8 on the same inputs bit for bit.
 * Plans: the split-key shapes only, as dta_attn_decode_rows (dta_decode_shared_supported tells
 * beforehand); anything else is DTA_ERR_UNSUPPORTED and the caller keeps the paged call.
 * Memory safety: len_b and every page id are clamped as in the paged call; a member index
 * outside [0, B) is an empty slot; rows_g is clamped to [0, shortest member's length]; no
 * table entry, page, scale or cache row at or past covered_g is read by the group pass and
 * nothing outside the members' slots is written.  An inconsistent plan (pages that are not
 * shared, a sequence in two groups) may give wrong numbers, never an out-of-range access.
 * Errors: everything the paged entry point rejects, and DTA_ERR_INVALID for n_groups < 0 or,
 * with n_groups > 0, a null or not 4-byte aligned plan pointer.  B*H == 0: DTA_OK, no launch;
 * n_groups == 0 is the paged call itself. */
typedef struct dta_attn_decode_paged_shared_args {
  int32_t dtype;
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;            /* host upper bound of every lengths_dev[b] (<= t_cap); sizes the grid */
  int32_t t_cap;             /* = max_pages * page_size; workspace row length */
  float scale;
  dta_tensor q, k_pool, v_pool, o;
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* lengths_dev;/* device int32 [B], required */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
  int32_t n_groups;
  const int32_t* group_members_dev;  /* device int32 [n_groups][8] */
  const int32_t* group_rows_dev;     /* device int32 [n_groups] */
} dta_attn_decode_paged_shared_args;
int dta_attn_decode_paged_shared(const dta_attn_decode_paged_shared_args* a, void* stream);

typedef struct dta_attn_decode_paged_shared_fp8_args {
  int32_t dtype;             /* of q and o */
  int32_t B, H, n_terms, head_size, dv;
  int32_t length;
  int32_t t_cap;
  float scale;
  dta_tensor q, k_pool, v_pool, o;   /* k_pool / v_pool: e4m3fn bytes, strides in bytes */
  const float* coef;         /* fp32 [h][i] */
  float* workspace;
  const int32_t* lengths_dev;/* device int32 [B], required */
  int32_t page_size, max_pages, n_pages;
  const int32_t* block_table_dev;  /* device int32 [B][max_pages] */
  const float* scale_pool_dev;     /* fp32 [page][row < P][h][N+1] */
  int64_t scale_page_stride;       /* floats from one page's scales to the next */
  int32_t n_groups;
  const int32_t* group_members_dev;  /* device int32 [n_groups][8] */
  const int32_t* group_rows_dev;     /* device int32 [n_groups] */
} dta_attn_decode_paged_shared_fp8_args;
int dta_attn_decode_paged_shared_fp8(const dta_attn_decode_paged_shared_fp8_args* a, void* stream);
int dta_decode_shared_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv, int32_t fp8_cache);

/* The row write of a ragged / paged step (still ABI 9; the presence of the symbol is the
 * capability check): the RoPE of a step's new rows and their scatter into the KV cache in one
 * launch.  In the reference those rows are recomputed with the whole prefix for every token
 * (diff_transformer.py:177-185; the rotation is Ndiff_transformer.py:11-22, 104-109); on the
 * KV cache they were a table gather, two dta_rope launches and an index_put_ of gathered
 * indices (kv_cache._seq_attention_step, write_rows).
 * q, k [b][t < Tn][h][i][d] and v [b][t < Tn][h][e] are the step's rows (strided views of the
 * packed projection).  For row r of sequence b
 *   at = clamp(pos_dev[b], 0, t_cap) + r,   real = r < count_dev[b] && at < t_cap
 *   q_out[b][r] = RoPE(q[b][r]) at table row min(at, t_cap - 1), for every row, padding rows
 *                 included (rope_freqs set; NULL: q_out is not touched, the caller keeps q)
 *   a real row:   K_i (rotated at table row `at` if rope_freqs is set) and V are stored to the
 *                 row's place, by dest
 *     DTA_KV_STEP_CONTIGUOUS  k_dst / v_dst [b][t < t_cap]...: row `at` of sequence b
 *     DTA_KV_STEP_PAGED       k_dst / v_dst a pool [page][row < P]...: row at % P of page
 *                             block_table_dev[b][at / P], the id clamped to [0, n_pages - 1]
 *                             before it forms an address
 *     DTA_KV_STEP_SLOTS       (an fp8 pool) nothing goes to a pool: the rotated K_i goes to
 *                             k_dst [b][r < Tn]... (a temporary; without rope_freqs k_dst is not
 *                             touched), v_dst is unused, and slots_out_dev[b * Tn + r] =
 *                             page * P + at % P, for a padding row n_pages * P + at % P, a slot
 *                             of the spare page: the slot_dev of dta_kv_quant_rows, which runs next
 *   a padding row stores no K and no V anywhere.
 * The rotation is dta_rope's, bit for bit (the same fp32 expressions in the same order).
 * rope_freqs is the whole fp32 [t_cap][head_size/2][2] table.  One thread moves 8 elements by
 * 16-byte accesses; every offset is 64-bit.
 * DTA_ERR_UNSUPPORTED: head_size or dv not a multiple of 8 (or above 128 / 256), n_terms > 8.
 * DTA_ERR_INVALID: dest outside the enum, t_cap < 1 or above 2^30, a null or not 4-byte aligned
 * pos_dev / count_dev, a view whose pointer or strides are not multiples of 16 bytes; paged and
 * slots: a page_size outside {32, 64, 128, 256}, n_pages < 1, max_pages * page_size < t_cap, a
 * null or misaligned block_table_dev (slots: slots_out_dev).  B * Tn == 0: DTA_OK, no launch. */
enum dta_kv_step_dest { DTA_KV_STEP_CONTIGUOUS = 0, DTA_KV_STEP_PAGED = 1, DTA_KV_STEP_SLOTS = 2 };
typedef struct dta_kv_step_rows_args {
  int32_t dtype;
  int32_t B, Tn, H, n_terms, head_size, dv;
  int32_t t_cap;             /* rows of a sequence's window: the table's rows, the bound of `at` */
  int32_t dest;              /* dta_kv_step_dest */
  int32_t page_size, max_pages, n_pages;   /* paged and slots (0 otherwise) */
  dta_tensor q, k, v;
  dta_tensor q_out;          /* as q; used with rope_freqs only */
  dta_tensor k_dst, v_dst;
  const float* rope_freqs;   /* fp32 [t_cap][head_size/2][2], or NULL */
  const int32_t* pos_dev;    /* device int32 [B] */
  const int32_t* count_dev;  /* device int32 [B] */
  const int32_t* block_table_dev;  /* device int32 [B][max_pages]; paged and slots */
  int32_t* slots_out_dev;    /* device int32 [B * Tn]; slots */
} dta_kv_step_rows_args;
int dta_kv_step_rows(const dta_kv_step_rows_args* a, void* stream);

/* Sampling: one token per logits row, in one launch (one 256-thread workgroup per row).  Replaces
 * softmax + multinomial of the generate loops where a sampler is asked for.  For row r, with
 * x_i = float(logits[r][i]) over V columns, T = temperature, k = top_k, p = top_p (the per-row
 * device value where the pointer is set, the scalar otherwise):
 *   degenerate   a row holding a NaN or a +inf, or all -inf: token -1, logprob NaN.  Every other row
 *                gives 0 <= token < V; nothing outside [-1, V) is ever written.
 *   m = max x_i.  T <= 0 (or a NaN device T): greedy, the lowest index with x_i == m, and
 *                logprob = x_t - m - log sum_i exp(x_i - m) (temperature 1, unfiltered).
 *   weights      z_i = (x_i - m) / T, w_i = exp(z_i), fp32
 *   top-k        off if k <= 0 or k >= V; i is kept iff #{j : x_j > x_i} < k (a tie class at the
 *                threshold is kept whole)
 *   top-p        off if p >= 1 or p <= 0 (or a NaN device p); among what top-k kept, i is kept iff
 *                sum_{j kept by k, x_j > x_i} w_j < p * sum_{j kept by k} w_j (the maximum always is;
 *                ties in or out together)
 *   draw         Z = sum of the kept w_i; the token is the lowest kept index whose inclusive prefix
 *                sum of kept weights, in index order, exceeds u * Z (the last kept index if rounding
 *                leaves none); logprob = z_t - log Z
 *   u            Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (offset lo, offset hi,
 *                stream lo, stream hi); u = (out[0] >> 8) * 2^-24.  No generator state, no host call.
 * A row's token and logprob are a bitwise function of the row, its parameters and (seed, stream,
 * offset): independent of R, of the row's index, of alignment and of timing (fixed-shape sums, no
 * floating-point atomics).  Any V in [1, 2^20], any row stride (elements); 16-byte loads where a
 * row starts 16-byte aligned, element loads otherwise.
 * DTA_ERR_INVALID: a null logits / token_out with R > 0, R < 0, V < 1, an unknown dtype, a NaN scalar
 * temperature / top_p, a per-row pointer not aligned to its element (4 bytes fp32 / int32, 8 bytes
 * int64).  DTA_ERR_UNSUPPORTED: V > 2^20.  R == 0: DTA_OK, no launch. */
typedef struct dta_sample_rows_args {
  int32_t dtype;
  int32_t R, V;
  const void* logits;
  int64_t row_stride;                /* elements */
  float temperature;                 /* the scalars: used where the per-row pointer is NULL */
  int32_t top_k;
  float top_p;
  const float* temperature_dev;      /* device [R], or NULL */
  const int32_t* top_k_dev;
  const float* top_p_dev;
  uint64_t seed;
  const int64_t* stream_dev;         /* device [R], or NULL: stream = row index */
  const int64_t* offset_dev;         /* device [R], or NULL: offset = 0 */
  int64_t* token_out;                /* device [R] */
  float* logprob_out;                /* device [R], or NULL */
} dta_sample_rows_args;
int dta_sample_rows(const dta_sample_rows_args* a, void* stream);

/* Sampling penalties: repetition / frequency / presence penalties, a logit bias (bans are a bias of -inf)
 * and the min-p floor of logits rows, in one launch (one 256-thread workgroup per row; still ABI 9, the
 * presence of the symbol is the capability check).  It writes fp32 rows that dta_sample_rows then samples.
 * Rows: R = B * Tn; row r is row j = r % Tn of sequence b = r / Tn.  Per sequence the device holds what the
 * speculative loop holds: hist[b][0 .. cap) and hlen_dev[b], optionally draft[b][0 .. K) and dcnt_dev[b],
 * and gen_start_dev[b], the prompt's length (NULL: 0).
 * Clamps, before anything is indexed:
 *   L = clamp(hlen, 0, cap)   g = clamp(gen_start, 0, L)   d = clamp(dcnt, 0, K) (0 without a draft)
 *   e = min(j, d)
 * The row's context is hist[b][0 .. L) followed by draft[b][0 .. e): what the plain loop has seen at that
 * position if the first j drafts are accepted (a row beyond an unaccepted draft is discarded anyway).  A
 * context token outside [0, V) is ignored.  For column i:
 *   s_i = 1 if i occurs anywhere in the context
 *   c_i = the occurrences of i at history positions >= g, plus those in the draft prefix
 * With x = float(logits[r][i]), theta = repetition, f = frequency, p = presence, gap = floor_gap (the
 * per-sequence device value where the pointer is set, the scalar otherwise), in this order, every
 * arithmetic operation one correctly rounded fp32 operation, nothing contracted:
 *   1. repetition   off at theta == 1 (or a NaN device theta).  If s_i: x = (x > 0) ? x / theta : x * theta;
 *                   the sign test is on the bits: -0 and +0 are not positive.
 *   2. frequency /  off at a NaN device f or p.  If c_i > 0: x = (x - f * float(c_i)) - p.
 *      presence
 *   3. bias         if bias is given: x = x + bias[b][i] (bias_stride 0: one row bias[i] shared by all).
 *   4. floor        min-p.  Off unless gap < 0 and finite.  m = the maximum over the row of the values
 *                   after step 3 that are not NaN; x = (x >= m + gap) ? x : -inf.  The caller passes
 *                   gap = fp32(T * ln(min_p)): the kernel sees neither T nor min_p.  A row whose m is
 *                   not finite is left as step 3 made it.
 * A NaN input is written through with its bits unchanged by every step.  (A NaN that the arithmetic
 * itself makes, inf - inf, is a NaN in the output; its payload is not specified.)
 * A row's output is a bitwise function of the row, its sequence's state and its parameters: independent of
 * B, of the row's index, of alignment and of timing.  Nothing outside out[r][0 .. V) is written -- not
 * the gap between rows where out_stride > V, and none of the inputs.
 * Counting: a per-row table of V 32-bit entries (the count in the low 31 bits, "seen before g" in the top
 * one), filled by integer atomics, which commute.  For V <= DTA_PENALTY_LDS_MAX_V (40944: 4 V bytes of
 * the CU's 160 KiB of LDS next to the kernel's 16 static bytes) it lives in LDS and no workspace is
 * needed; beyond, in `workspace`, dta_penalize_rows_workspace_bytes(R, V) = 4 R V bytes (0 on the LDS
 * path), of whose contents nothing is assumed.  No floating-point atomics; 64-bit address arithmetic.
 * Any V in [1, 2^20], any row strides (elements); vector accesses where a row starts aligned to them,
 * element accesses otherwise.
 * DTA_ERR_INVALID: B < 0, Tn < 0, B * Tn above 2^31 - 1, V < 1, an unknown dtype, cap outside 1 .. 2^30,
 * K outside 0 .. 7, a row stride below its row (row_stride < V, out_stride < V, hist_stride < cap,
 * draft_stride < K with a draft, bias_stride neither 0 nor >= V), a null logits / out / hist / hlen_dev
 * with R > 0, draft without dcnt_dev or the reverse, a pointer not aligned to its element, a NaN scalar
 * parameter, repetition <= 0, a workspace that is null or smaller than the query says where one is
 * needed.  DTA_ERR_UNSUPPORTED: V > 2^20.  R == 0: DTA_OK, no launch. */
#define DTA_PENALTY_LDS_MAX_V 40944
typedef struct dta_penalize_rows_args {
  int32_t dtype;
  int32_t B, Tn, V;
  int32_t cap;                       /* tokens a row of hist holds */
  int32_t K;                         /* tokens a row of draft holds, 0 .. 7 */
  const void* logits;                /* device [B * Tn][V], dtype */
  int64_t row_stride;                /* elements */
  float* out;                        /* device fp32 [B * Tn][V] */
  int64_t out_stride;
  const int32_t* hist;               /* device int32 [B][cap] */
  int64_t hist_stride;
  const int32_t* hlen_dev;           /* device int32 [B] */
  const int32_t* gen_start_dev;      /* device int32 [B], or NULL: 0 */
  const int32_t* draft;              /* device int32 [B][K], or NULL */
  int64_t draft_stride;
  const int32_t* dcnt_dev;           /* device int32 [B]; with draft */
  float repetition, frequency, presence, floor_gap;   /* used where the per-sequence pointer is NULL */
  const float* repetition_dev;       /* device fp32 [B], or NULL */
  const float* frequency_dev;
  const float* presence_dev;
  const float* floor_gap_dev;
  const float* bias;                 /* device fp32 [B][V] or [V], or NULL */
  int64_t bias_stride;               /* elements; 0: one shared row */
  void* workspace;                   /* device, dta_penalize_rows_workspace_bytes(B * Tn, V) bytes; may be NULL at 0 */
  size_t workspace_bytes;
} dta_penalize_rows_args;
size_t dta_penalize_rows_workspace_bytes(int64_t R, int32_t V);
int dta_penalize_rows(const dta_penalize_rows_args* a, void* stream);

/* Speculative decoding: one round's acceptance and the next prompt-lookup draft in one launch (still
 * ABI 9; the presence of the symbol is the capability check).  One 256-thread workgroup per sequence.
 * The draft is deterministic, so exact speculative sampling is: draw t from the target distribution
 * with the uniform the plain loop would use at that position (dta_sample_rows with stream b and
 * offset = tokens emitted so far + j), accept draft token d iff t == d, otherwise emit t.  The tokens
 * emitted are therefore the plain loop's, whatever was drafted.
 * State of sequence b (device int32, owned by the caller's loop, updated in place):
 *   hist[b][0 .. cap)    token history; hlen_dev[b] tokens of it are set, the last one is pending:
 *                        emitted, not yet through the model
 *   remaining_dev[b]     new tokens still owed; <= 0: finished
 *   draft[b][0 .. K)     the draft the round verified, dcnt_dev[b] tokens of it
 * Input: tok[b][0 .. Tn), int64, the samples of the round's logits rows: row 0 follows the pending
 * token, row j follows draft[j - 1].  0 <= Tn <= K + 1 (Tn = 0: no rows to accept, a draft alone).
 * Clamps, before anything is indexed: hlen into [0, cap], dcnt into [0, min(K, max(Tn - 1, 0))].
 * Accept.
 *   1. remaining <= 0: the row is left alone (no byte of its state is written): m = 0, next dcnt = 0.
 *   2. a = #{leading j < dcnt : tok[b][j] == draft[b][j]},  m = min(a + 1, remaining, Tn, cap - hlen)
 *      (the last term keeps the append inside hist; a caller that sizes cap >= hlen + remaining
 *      never meets it).
 *   3. The emitted tokens are tok[b][0 .. m).
 *   4. If one of them is eos_id or negative (the sampler's -1 for a degenerate row), m is cut to end
 *      just after the first such token and remaining becomes 0; otherwise remaining -= m.
 *   5. hist[b][hlen .. hlen + m) = the emitted tokens (as int32), hlen += m.
 *   6. The KV cache keeps m of the round's rows, the pending token's and the m - 1 accepted drafts':
 *      the caller truncates it to its old length + m.
 * Draft (L = the new hlen, remaining the new one).
 *   1. ngram_min == 0 (lookup off: the caller drafts), remaining <= 1 or L <= ngram_min: dcnt = 0.
 *   2. For each end e in [ngram_min - 1, L - 1): mu(e) = the largest n <= min(ngram_max, e + 1) with
 *      hist[e - t] == hist[L - 1 - t] for all t < n.
 *   3. Among the ends with mu(e) >= ngram_min the one maximising (mu(e), e) wins -- the longest
 *      match, then the latest -- found as one 64-bit integer maximum of (mu << 32 | e).
 *   4. dcnt = max(0, min(K, L - 1 - e, remaining - 1, t_cap - L)), draft[b][0 .. dcnt) =
 *      hist[e + 1 ..); no such end: dcnt = 0.  Draft entries at and beyond dcnt are not written.
 * result_out[b] = (m, dcnt), int32 [B][2]: what the host reads back once a round.
 * A row's outputs are a function of the row alone: independent of B, of the row's index and of
 * timing (integers only, no atomics).  Nothing outside hist[b][hlen .. hlen + m), draft[b][0 .. dcnt),
 * the three scalars of an unfinished row and result_out[b] is written.
 * DTA_ERR_INVALID: B < 0, K outside 1 .. 7, Tn outside 0 .. K + 1, ngram_max outside 1 .. 8,
 * ngram_min outside 0 .. ngram_max, cap or t_cap outside 1 .. 2^30, a row stride below its row
 * (hist_stride < cap, draft_stride < K, tok_stride < Tn), a null pointer (tok may be null at Tn = 0)
 * or one not aligned to its element.  B == 0: DTA_OK, no launch. */
typedef struct dta_spec_accept_draft_args {
  int32_t B, Tn, K;
  int32_t cap;                       /* tokens a row of hist holds */
  int32_t t_cap;                     /* the model's window (block_size): bounds a draft */
  int32_t ngram_min, ngram_max;      /* ngram_min 0: no lookup */
  int32_t eos_id;                    /* or -1 */
  int64_t hist_stride, draft_stride, tok_stride;   /* elements from one row to the next */
  int32_t* hist;                     /* device int32 [B][cap] */
  int32_t* hlen_dev;                 /* device int32 [B] */
  int32_t* remaining_dev;            /* device int32 [B] */
  int32_t* draft;                    /* device int32 [B][K] */
  int32_t* dcnt_dev;                 /* device int32 [B] */
  const int64_t* tok;                /* device int64 [B][Tn] */
  int32_t* result_out;               /* device int32 [B][2] */
} dta_spec_accept_draft_args;
int dta_spec_accept_draft(const dta_spec_accept_draft_args* a, void* stream);

/* A fixed-shape speculative round: the two pieces of glue that let one round -- always K + 1 rows per
 * sequence -- be captured as a graph and replayed, no host value shaping it (still ABI 9; the presence
 * of each symbol is the capability check).  Integers only, 64-bit address arithmetic, no atomics; every
 * device value is clamped before it forms an address.
 *
 * dta_spec_feed_rows builds the round's model inputs from the state dta_spec_accept_draft keeps.
 * Per sequence b, with T = K + 1:
 *   L      = clamp(hlen_dev[b], 0, cap)
 *   live   = remaining_dev[b] > 0 && L >= 1
 *   d      = live ? clamp(dcnt_dev[b], 0, K) : 0
 *   counts_out[b]    (int32) = live ? d + 1 : 0
 *   idx_out[b][0]    (int64) = live ? clamp(hist[b][L - 1], 0, vocab - 1) : 0      the pending token
 *   idx_out[b][j]    (int64) = j <= d ? clamp(draft[b][j - 1], 0, vocab - 1) : 0   for 1 <= j <= K
 *   offset_out[b][j] (int64) = (int64)total - (int64)remaining_dev[b] + j          for 0 <= j < T
 * total is the call's number of new tokens, so offset_out[b][j] is the dta_sample_rows offset of the
 * plain loop at that position (tokens emitted so far + j); the difference is taken in 64 bits, so no
 * device value overflows it.  All T entries of idx_out[b] and offset_out[b] are written, padding
 * included: a replay never reads a stale value.  hist[b][L - 1] is loaded only for a live row and
 * draft[b][j - 1] only for j <= d.  Nothing else is written; a row's outputs are a function of the row
 * alone.
 * DTA_ERR_INVALID: B < 0, K outside 1 .. 7, vocab < 1, total < 0, cap outside 1 .. 2^30, a row stride
 * below its row (hist_stride < cap, draft_stride < K, idx_stride < K + 1, offset_stride < K + 1), a
 * null pointer or one not aligned to its element.  B == 0: DTA_OK, no launch. */
typedef struct dta_spec_feed_rows_args {
  int32_t B, K;
  int32_t cap;                       /* tokens a row of hist holds */
  int32_t vocab;                     /* tokens are clamped into [0, vocab - 1] */
  int32_t total;                     /* the call's max_new_tokens */
  int64_t hist_stride, draft_stride, idx_stride, offset_stride;   /* elements from one row to the next */
  const int32_t* hist;               /* device int32 [B][cap] */
  const int32_t* hlen_dev;           /* device int32 [B] */
  const int32_t* remaining_dev;      /* device int32 [B] */
  const int32_t* draft;              /* device int32 [B][K] */
  const int32_t* dcnt_dev;           /* device int32 [B] */
  int64_t* idx_out;                  /* device int64 [B][K + 1] */
  int32_t* counts_out;               /* device int32 [B] */
  int64_t* offset_out;               /* device int64 [B][K + 1] */
} dta_spec_feed_rows_args;
int dta_spec_feed_rows(const dta_spec_feed_rows_args* a, void* stream);

/* dta_spec_commit_lengths is the device half of the cache's roll-back: the round's model step leaves
 * the cache lengths where they were, and this launch, their only writer in a round, advances each by
 * what dta_spec_accept_draft emitted.  For each b:
 *   s = slots ? clamp(slots[b], 0, n_slots - 1) : b
 *   lengths[s] = min(lengths[s] + clamp(result[b][0], 0, K + 1), t_cap)      (the sum in 64 bits)
 * result is dta_spec_accept_draft's result_out, int32 [B][2], packed.  The caller guarantees that the
 * slots are distinct; an entry of lengths that no b names is not touched.
 * DTA_ERR_INVALID: B < 0, K outside 1 .. 7, t_cap outside 1 .. 2^30, n_slots < 1, n_slots < B without
 * slots, a null lengths or result, a pointer not aligned to its element.  B == 0: DTA_OK, no launch. */
typedef struct dta_spec_commit_lengths_args {
  int32_t B, K;
  int32_t t_cap;                     /* the model's window: no length passes it */
  int32_t n_slots;                   /* entries of lengths */
  int32_t* lengths;                  /* device int32 [n_slots] */
  const int32_t* result;             /* device int32 [B][2]: (m, next dcnt) */
  const int64_t* slots;              /* device int64 [B], or null: sequence b is entry b */
} dta_spec_commit_lengths_args;
int dta_spec_commit_lengths(const dta_spec_commit_lengths_args* a, void* stream);

/* SwiGLU of the Block feed-forward (diff_transformer.py SwiGLU.forward,
 * Ndiff_transformer.py:86-93 equivalent, control.py:80-90): out = silu(a) * b over
 * rows x n elements (n % 8 == 0; every row stride a multiple of 8 elements, every
 * pointer 16-byte aligned), and its backward da = dout * b * silu'(a),
 * db = dout * silu(a).  Unused pointers of the other direction may be NULL. */
typedef struct {
  int32_t dtype;
  int64_t rows, n;
  const void* a; int64_t a_stride;
  const void* b; int64_t b_stride;
  void* out; int64_t out_stride;
  const void* dout; int64_t dout_stride;
  void* da; int64_t da_stride;
  void* db; int64_t db_stride;
  /* backward, optional (ABI 3): with dbias, also the column sums of dA | dB as stored
   * (fp32 [2n]: the gate / xform Linears' bias gradient), through dbias_work
   * (dta_swiglu_bwd_workspace_bytes), summed in a fixed order */
  float* dbias; float* dbias_work;
} dta_swiglu_args;
int dta_swiglu_fwd(const dta_swiglu_args* a, void* stream);
int dta_swiglu_bwd(const dta_swiglu_args* a, void* stream);
size_t dta_swiglu_bwd_workspace_bytes(int64_t rows, int64_t n);

/* dst[i] += (float)src[i], i < n: gradient accumulation of a bf16/fp16/fp32 weight
 * gradient into fp32 master-gradient storage (the training step's packed projection
 * weights, SURVEY 8e/8f: torch.autograd's AccumulateGrad of the reference's
 * nn.Linear parameters, train.py:251-279).  src and dst 16-byte aligned. */
int dta_accumulate_f32(int32_t dtype, int64_t n, const void* src, float* dst, void* stream);

/* Cast/copy a [b][t][h][i][d] tensor from fp32 to dtype (dQ finalisation). */
int dta_cast_f32(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t n_terms,
                 int32_t head_size, const float* src, dta_tensor dst, void* stream);

const char* dta_error_string(int code);
int dta_abi_version(void);
/* 1 if (dtype, head_size, n_terms, dv) runs: an n_terms-branch kernel plan is built for
 * it, or (n_terms >= 2, dv = 2*head_size) the single-branch plan is -- then the forward
 * runs n_terms single-branch workgroups per query block and head plus a combine pass.
 * The backward runs each stage as branch groups of the largest built branch count not
 * above that stage's cap (group_max_dq / group_max_dkdv and their defaults), one launch
 * per group (dV summed over the groups, d(coef) reduced over all n_terms); where the two
 * stages group differently the DQ stage re-bases the delta rows for the DKDV stage.  Head sizes
 * 16, 32, 64, 96, 128 (dv = 2*head_size), and dv = head_size at n_terms = 1 for 32, 64,
 * 96, 128; the Python layer runs other head sizes up to 128 zero-padded to the next one. */
int dta_supported(int32_t dtype, int32_t head_size, int32_t n_terms, int32_t dv);

#ifdef __cplusplus
}
#endif
#endif /* DIFFATTN_H_ */
