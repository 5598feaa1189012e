// decode.hip -- one-query-row (and, split-key plan, up to eight-row) differential attention over a KV cache, gfx950.
//
// The reference's generate() (diff_transformer.py:177-185, Ndiff_transformer.py
// generate, control.py:163-171) re-runs the whole prefix for every new token.
// With a KV cache only the new token's row of the attention is needed:
//   o = sum_i coef[h][i] * softmax(q_i K_i[0:L]^T * scale) V[0:L]
// This is HBM-bound (each cached K_i / V row is read once per token), so the
// kernel is plain vector code, not MFMA: one workgroup per (b, h), four waves.
//   phase 1  every thread scores whole keys (16-byte K loads, q_i in LDS),
//            scores -> fp32 workspace, per-branch block max
//   phase 2  e = exp(s - m_i) in place, per-branch block sum l_i
//   phase 3  w_j = sum_i coef_i e_ij / l_i (the combined map row)
//   phase 4  o[e] = sum_j w_j V[j][e]: threads own a column, key groups stride
//            (coalesced V rows), LDS reduction over the groups.
// The split-key plan below is the one used for the standard head sizes.
// Algorithmic bytes per (b, h) and token: L * (N*hs + dv) * sizeof(E).
// Ragged batches (dta_attn_decode_ragged) run the same kernels with L read per
// sequence (clamp_len): L = len_b above, and a length of 0 writes zeros.
// Paged caches (dta_attn_decode_paged) are the PG = true instantiations of the same
// kernels: key row j of sequence b is row j % P of pool page table[b][j / P].  The
// chunk is a whole number of pages, so the split kernel looks its (at most chunk / 32)
// page ids up once, into LDS; every load, product and reduction after the address is
// the unpaged kernel's, in the same order, so the outputs are bitwise equal.
#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

template <class E>
__device__ __forceinline__ void ld8f(const E* p, float* f) {
  if constexpr (sizeof(E) == 2) {
    typedef E v8 __attribute__((ext_vector_type(8)));
    const v8 v = *reinterpret_cast<const v8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
  } else {
    const f32x4* q = reinterpret_cast<const f32x4*>(p);
    const f32x4 a = q[0], b = q[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[j + 4] = b[j]; }
  }
}

// ---- fp8 cache rows (dta_attn_decode_paged_fp8) -------------------------------------
// The cache element type C is a template parameter next to E (the type of q and o).  With
// C = E every expression below is the one it was; C = f8e4 reads OCP e4m3fn bytes
// (v_cvt_pk_f32_fp8) and one fp32 scale per (row, head, K_i | V) from kvs:
//   score_ij = (q_i . byte(K_i[j])) * k_scale[j][h][i]     one multiply per (row, branch)
//   acc_i   += (e_ij * v_scale[j][h]) * byte(V[j])          the row sum l_i keeps e_ij
// The split kernel asks for the scales of a chunk once, thread = key, before phase 1, and applies
// both in phase 2, where a thread owns a key anyway.  A lane reads kF8KB bytes of a K row
// and kF8VB bytes of a V row (8 or 16: the A/B is in DESIGN.md).  Rows >= len_b, their
// scales included, are never loaded.
constexpr int kF8KB = 16;
constexpr int kF8VB = 8;   // 16 doubles the V row groups and `part`, and halves the occupancy: slower (A/B)
static_assert((kF8KB == 8 || kF8KB == 16) && (kF8VB == 8 || kF8VB == 16), "8 or 16 bytes per lane");

// n (8 or 16) cache elements at p as floats
template <class C, int n>
__device__ __forceinline__ void ldnf(const C* p, float* f) {
  if constexpr (is_f8<C>) {
    typedef uint32_t uv __attribute__((ext_vector_type(n / 4)));
    const uv v = *reinterpret_cast<const uv*>(p);
#pragma unroll
    for (int w = 0; w < n / 4; ++w) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], true);
      f[4 * w] = lo[0]; f[4 * w + 1] = lo[1]; f[4 * w + 2] = hi[0]; f[4 * w + 3] = hi[1];
    }
  } else {
    static_assert(n == 8, "16- and 32-bit caches are read 8 elements per lane");
    ld8f<C>(p, f);
  }
}
template <class C>
__device__ __forceinline__ float ld1f(const C* p) {
  if constexpr (is_f8<C>) return __builtin_amdgcn_cvt_f32_fp8((int)p->b, 0);
  else return (float)*p;
}
// the N + 1 scales of cache row j of sequence b, head h (paged only)
__device__ __forceinline__ const float* scale_row(const DecodeParams& p, int page, int r, int h, int N) {
  return p.kvs + (int64_t)page * p.kvs_sb + ((int64_t)r * p.H + h) * (N + 1);
}

__device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide reduction of NB per-thread values (all threads get the result)
template <int NB, bool MAX>
__device__ __forceinline__ void block_reduce(float (&v)[NB], float* red) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const float r = MAX ? wmax(v[i]) : wsum(v[i]);
    if (lane == 0) red[wave * NB + i] = r;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    float r = red[i];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = MAX ? fmaxf(r, red[w * NB + i]) : r + red[w * NB + i];
    v[i] = r;
  }
  __syncthreads();
}

// The valid length of sequence b: the device value when given (one for the launch,
// Lsb = 0, or one per sequence, Lsb = 1: ragged batches), clamped to [0, L] (L = the
// host upper bound the grid and workspace were sized for), so a bad device length can
// never index past the cache, the workspace or the combine's LDS weights.
__device__ __forceinline__ int clamp_len(const DecodeParams& p, int b) {
  return p.Ldev ? min(max(p.Ldev[b * p.Lsb], 0), p.L) : p.L;
}

// element offset of cache row j of sequence b in the k / v view t (head and branch excluded)
template <bool PG>
__device__ __forceinline__ int64_t row_off(const DecodeParams& p, const T5& t, int b, int j) {
  if constexpr (PG) return (int64_t)page_of(p.pg, b, j) * t.sb + (int64_t)(j & ((1 << p.pg.shift) - 1)) * t.st;
  else return b * t.sb + (int64_t)j * t.st;
}

template <class E, int N, bool PG, class C>
__global__ __launch_bounds__(kThreads) void decode_kernel(DecodeParams p) {
  constexpr bool F8 = is_f8<C>;
  static_assert(!F8 || PG, "the fp8 cache is a paged cache");
  __shared__ float qs[N * 128];
  __shared__ float red[kWaves * N];
  __shared__ float part[kThreads];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int HS = p.HS, DV = p.DV, L = clamp_len(p, b);
  const E* gq = reinterpret_cast<const E*>(p.q.p) + b * p.q.sb + h * p.q.sh;
  for (int x = tid; x < N * HS; x += kThreads) qs[x] = (float)gq[(x / HS) * p.q.si + x % HS];
  __syncthreads();

  float* ws = p.ws + ((int64_t)b * p.H + h) * N * p.ldw;     // [i][ldw]
  const C* gk = reinterpret_cast<const C*>(p.k.p) + h * p.k.sh;
  [[maybe_unused]] const int pmask = (1 << p.pg.shift) - 1;
  float m[N];
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = -INFINITY;
  for (int j = tid; j < L; j += kThreads) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const C* kr = gk + row_off<PG>(p, p.k, b, j) + i * p.k.si;
      float s = 0.f;
      for (int d = 0; d < HS; d += 8) {
        float f[8];
        ldnf<C, 8>(kr + d, f);
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(qs[i * HS + d + u], f[u], s);
      }
      if constexpr (F8) s *= p.scale * scale_row(p, page_of(p.pg, b, j), j & pmask, h, N)[i];
      else s *= p.scale;
      ws[i * p.ldw + j] = s;
      m[i] = fmaxf(m[i], s);
    }
  }
  block_reduce<N, true>(m, red);

  float l[N];
#pragma unroll
  for (int i = 0; i < N; ++i) l[i] = 0.f;
  for (int j = tid; j < L; j += kThreads)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float e = __expf(ws[i * p.ldw + j] - m[i]);
      ws[i * p.ldw + j] = e;
      l[i] += e;
    }
  block_reduce<N, false>(l, red);

  float c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = p.coef[h * N + i] / l[i];
  for (int j = tid; j < L; j += kThreads) {
    float w = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) w = fmaf(c[i], ws[i * p.ldw + j], w);
    if constexpr (F8) w *= scale_row(p, page_of(p.pg, b, j), j & pmask, h, N)[N];   // V's scale, after the l_i
    ws[j] = w;                                  // row 0 now holds the combined map row
  }
  __threadfence_block();
  __syncthreads();

  // phase 4: G key groups x DV columns
  const int G = kThreads / DV;
  const int g = tid / DV, e = tid % DV;
  const C* gv = reinterpret_cast<const C*>(p.v.p) + h * p.v.sh + e;
  float acc = 0.f;
  if (g < G)
    for (int j = g; j < L; j += G) acc = fmaf(ws[j], ld1f<C>(gv + row_off<PG>(p, p.v, b, j)), acc);
  part[tid] = acc;
  __syncthreads();
  if (tid < DV) {
    float o = 0.f;
    for (int x = 0; x < G; ++x) o += part[x * DV + tid];
    E* go = reinterpret_cast<E*>(p.o.p) + b * p.o.sb + h * p.o.sh;
    go[tid] = (E)o;
  }
}

// ---- split-key path (flash-decoding): fills the chip when B*H is small ------
// Grid (S, H, B): workgroup s owns keys [s*kChunk, (s+1)*kChunk).  It writes,
// per branch i, the chunk's max m_i, sum l_i = sum_j exp(s_ij - m_i) and the
// un-normalised row acc_i = sum_j exp(s_ij - m_i) V_j (fp32).  decode_combine
// rescales the S partials to the global max and applies coef_i / L_i.
// K rows are read by LPR = HS/8 lanes each (one 16-byte load per lane), V rows
// by DV/8 lanes each, so every wave-level load is a run of whole rows.  (fp8 cache:
// HS / kF8KB and DV / kF8VB lanes, one 8- or 16-byte load per lane.)
// kChunk: keys per split workgroup.  DTA_DECODE_CHUNK (256) sizes the workspace
// (the most splits); launches with >= kWideGrid workgroups use 2x chunks, which
// halves the partials (A/B: +4.5% at B=8 H=16 L=32768, slower on smaller grids)
constexpr int kWideGrid = 8192;

// ---- several query rows per launch (dta_attn_decode_rows*) --------------------------
// R > 1 instantiates the same two kernels for a step of Tq <= kMaxRows new rows per sequence:
// query row r of sequence b sits at pos_b + r and is the one-row decode at length pos_b + r + 1.
// A workgroup loads every K and V row of its chunk once (rows < pos_b + count_b only) and
// carries R rows through the three phases at a time: R query vectors and R accumulators per
// lane, R * N score rows in LDS.  Where R < count_b the rows go in passes of R (the later
// passes find the chunk in cache).  Row r masks the keys >= its own length exactly where the
// one-row kernel masks the keys >= L (score -inf, probability 0), so its max, its sums and
// its accumulators see the same operands in the same order; the keys between its length and
// the step's end enter its accumulators as fmaf(0, v, acc) with v a real row of this step.
// `part` is reused row by row for the cross-group sum and shares its LDS with the scores,
// which are dead by then.  With R = 1 every expression below is the one-row kernel's.
constexpr int kMaxRows = 8;
// rows per pass: the most (of 8, 4, 2) whose query vectors and accumulators stay in registers
template <int N, class C>
constexpr int rows_per_pass() {
  constexpr int per = N * (is_f8<C> ? (kF8KB > kF8VB ? kF8KB : kF8VB) : 8);
  return per * 8 <= 128 ? 8 : per * 4 <= 128 ? 4 : 2;
}
// sequence b's step: position of query row 0 and number of real rows, clamped so that no
// device value can index past the cache, the workspace or LDS (the extend kernels' clamps)
struct RowSpan { int pos, cnt; };
__device__ __forceinline__ RowSpan row_span(const DecodeParams& p, int b) {
  RowSpan r;
  r.pos = min(max(p.pos_dev[b], 0), p.ldw - p.Tq);
  r.cnt = p.cnt_dev ? min(max(p.cnt_dev[b], 0), p.Tq) : p.Tq;
  return r;
}

// ---- shared-prefix plan (dta_attn_decode_paged_shared*) -----------------------------------
// SH instantiates the R > 1 kernel once more, for the one-row step of a batch in which groups
// of 2 .. kShared sequences have the same pool pages under their first rows (forks of one
// prompt): the R rows of a pass are R member sequences of group blockIdx.z, not R consecutive
// rows of one sequence.  A workgroup runs only for a chunk that lies wholly below the group's
// covered rows (a multiple of the chunk, at most the shortest member's length), looks the pages
// up in the first member's table, loads K, V and the scales once, and writes each member's
// partial into that member's own one-row slot [b][h][s].  No row is masked (the chunk is below
// every member's length), so every operand and every order is the one-row kernel's on a full
// chunk.  The one-row pass that follows on the same stream (OWN: the R = 1 kernel with one early
// exit more) skips the chunks of a sequence below its group's covered rows (own_covered), and
// the one-row combine reduces what it finds.
constexpr int kShared = 8;                    // member slots per group
struct SharedGroup { int first, covered; };   // first valid member (-1: none), covered rows
// Every device value is clamped before use: a member outside [0, B) is an empty slot, the rows
// lie in [0, shortest member's clamped length], so nothing at or past `covered` is ever read.
template <int kChunk>
__device__ __forceinline__ SharedGroup shared_group(const DecodeParams& p, int g) {
  SharedGroup r{-1, 0};
  int lo = p.L;
  for (int x = kShared - 1; x >= 0; --x) {
    const int m = p.sh_mem[g * kShared + x];
    if (m >= 0 && m < p.B) { lo = min(lo, clamp_len(p, m)); r.first = m; }
  }
  r.covered = min(max(p.sh_rows[g], 0), lo) / kChunk * kChunk;
  return r;
}
// the rows of sequence b the group pass covered (0: b is in no group); `grp` is one LDS word
template <int kChunk>
__device__ __forceinline__ int own_covered(const DecodeParams& p, int b, int* grp) {
  if (threadIdx.x == 0) *grp = -1;
  __syncthreads();
  for (int x = threadIdx.x; x < p.sh_g * kShared; x += kThreads)
    if (p.sh_mem[x] == b) *grp = x / kShared;
  __syncthreads();
  const int g = *grp;
  return g < 0 ? 0 : shared_group<kChunk>(p, g).covered;
}

// MODE 0: the kernels of every other entry point; 1: the group pass (SH); 2: the one-row pass of a
// shared-prefix step (OWN), instantiations of their own so that the MODE 0 kernels stay as they are
template <class E, int N, int HS, int DV, int kChunk, bool PG, class C, int R, int MODE = 0>
__global__ __launch_bounds__(kThreads) void decode_split_kernel(DecodeParams p) {
  constexpr bool F8 = is_f8<C>;
  constexpr bool ROWS = R > 1;
  constexpr bool SH = MODE == 1, OWN = MODE == 2;
  static_assert(!F8 || PG, "the fp8 cache is a paged cache");
  static_assert(!SH || (PG && ROWS && kShared % R == 0), "the group pass is a paged multi-row pass");
  static_assert(!OWN || (PG && !ROWS), "the own pass is the paged one-row pass");
  constexpr int KE = F8 ? kF8KB : 8;          // K elements per lane
  constexpr int VE = F8 ? kF8VB : 8;          // V elements per lane
  constexpr int LPR = HS / KE;                // lanes per K row
  constexpr int KPW = 64 / LPR;               // keys per wave per load
  constexpr int VPR = DV / VE;                // lanes per V row
  constexpr int G = kThreads / VPR;           // V row groups
  constexpr int KPT = kChunk / kThreads;      // keys per thread in the softmax phase
  static_assert(kChunk % kThreads == 0, "chunk must be a multiple of the workgroup");
  constexpr int kSc = R * N * kChunk, kPart = G * N * (DV + 4);
  __shared__ float lds[ROWS ? (kSc > kPart ? kSc : kPart) : kSc + kPart];
  float (*sc)[N][kChunk] = reinterpret_cast<float (*)[N][kChunk]>(lds);                        // [R][N][kChunk]
  float (*part)[N][DV + 4] = reinterpret_cast<float (*)[N][DV + 4]>(lds + (ROWS ? 0 : kSc));   // [G][N][DV + 4]
  __shared__ float red[kWaves * N * R];
  __shared__ int pgs[PG ? kChunk / 32 : 1];   // paged: the chunk's pool pages (page size >= 32)
  const int s = blockIdx.x, h = blockIdx.y;
  int b = blockIdx.z;                          // group pass: the group, then its first member (the table read)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = s * kChunk;
  // L: the keys the workgroup may load (rows: up to the step's last real row; none without one;
  // group pass: the group's covered rows, a multiple of the chunk)
  int pos = 0, cnt = 1, L;
  [[maybe_unused]] const int* mem = nullptr;   // group pass: the group's kShared member slots
  if constexpr (SH) {
    const SharedGroup sg = shared_group<kChunk>(p, b);
    if (sg.first < 0) return;
    mem = p.sh_mem + b * kShared;
    b = sg.first;
    cnt = kShared;
    L = sg.covered;
  } else if constexpr (ROWS) {
    const RowSpan sp = row_span(p, b);
    pos = sp.pos; cnt = sp.cnt;
    L = cnt ? pos + cnt : 0;
  } else {
    L = clamp_len(p, b);
  }
  if (j0 >= L) return;                         // grid sized for an upper bound; a chunk past its own
                                               // sequence's length touches no memory (uniform exit)
  if constexpr (OWN) {
    // shared-prefix plan: the group pass wrote this chunk's partial (uniform exit, before any cache load)
    if (j0 < own_covered<kChunk>(p, b, reinterpret_cast<int*>(red))) return;
  }
  const int nk = min(kChunk, L - j0);
  // paged: the chunk starts on a page boundary (page size divides kChunk); only the pages
  // that hold a row below L are looked up (the rest of the table may hold anything)
  [[maybe_unused]] const int psh = p.pg.shift, pmask = (1 << psh) - 1;
  if constexpr (PG) {
    if (tid < kChunk / 32) pgs[tid] = (tid << psh) < nk ? page_of(p.pg, b, j0 + (tid << psh)) : 0;
    __syncthreads();
  }
  // element offset of chunk row jj (< nk) in the view t
  auto crow = [&](const T5& t, int jj) -> int64_t {
    if constexpr (PG) return (int64_t)pgs[jj >> psh] * t.sb + (int64_t)(jj & pmask) * t.st;
    else return b * t.sb + (int64_t)(j0 + jj) * t.st;
  };

  // fp8: the scales of this thread's phase-2 keys (K_i: [0, N), V: [N]), asked for here so that
  // they arrive under the K stream; after the early exit and the page list, as every load is
  [[maybe_unused]] float ksc[F8 ? KPT : 1][N + 1];
  if constexpr (F8) {
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const int j = tid + r * kThreads;
      const float* sp = scale_row(p, pgs[min(j, nk - 1) >> psh], j & pmask, h, N);
#pragma unroll
      for (int x = 0; x <= N; ++x) ksc[r][x] = j < nk ? sp[x] : 0.f;
    }
  }

  // rows: passes of R rows (one pass, cnt = 1, for the one-row kernel)
  for (int r0 = 0; r0 < cnt; r0 += R) {
  const int nr = ROWS ? min(R, cnt - r0) : 1;   // real rows of this pass
  // group pass: the member sequence behind row x (-1: an empty slot, which is no row)
  [[maybe_unused]] int bx[R];
  if constexpr (SH) {
    bool any = false;
#pragma unroll
    for (int x = 0; x < R; ++x) {
      const int m = mem[r0 + x];
      bx[x] = m >= 0 && m < p.B ? m : -1;
      any |= bx[x] >= 0;
    }
    if (!any) continue;                         // uniform
  }
  auto live = [&](int x) -> bool {
    if constexpr (SH) return bx[x] >= 0;
    else return x < nr;
  };
  // nkr[x]: the keys of this chunk that row x attends to (0: the chunk lies past the row, or no row)
  int nkr[R];
#pragma unroll
  for (int x = 0; x < R; ++x)
    nkr[x] = SH ? (live(x) ? nk : 0) : ROWS ? (x < nr ? min(max(pos + r0 + x + 1 - j0, 0), nk) : 0) : nk;
  if constexpr (ROWS && !SH) {
    if (pos + r0 + nr <= j0) continue;          // the chunk lies past every row of the pass (uniform)
  }

  // phase 1: scores of this chunk into LDS
  {
    const int sub = lane % LPR, kr = lane / LPR;
    const E* gq = reinterpret_cast<const E*>(p.q.p) + (SH ? 0 : b * p.q.sb) + h * p.q.sh + sub * KE;
    float q[R][N][KE];
#pragma unroll
    for (int x = 0; x < R; ++x) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (live(x)) {
          const E* gx = SH ? gq + bx[x] * p.q.sb : ROWS ? gq + (int64_t)(r0 + x) * p.q.st : gq;
#pragma unroll
          for (int c = 0; c < KE; c += 8) ld8f<E>(gx + i * p.q.si + c, q[x][i] + c);
#pragma unroll
          for (int u = 0; u < KE; ++u) q[x][i][u] *= p.scale;
        } else {
#pragma unroll
          for (int u = 0; u < KE; ++u) q[x][i][u] = 0.f;
        }
      }
    }
    const C* gk = reinterpret_cast<const C*>(p.k.p) + h * p.k.sh + sub * KE;
    for (int jj = wave * KPW + kr; jj < kChunk; jj += kWaves * KPW) {
      const bool ok = jj < nk;
      const C* kp = gk + crow(p.k, ok ? jj : 0);
      float f[N][KE];
#pragma unroll
      for (int i = 0; i < N; ++i) ldnf<C, KE>(kp + i * p.k.si, f[i]);
#pragma unroll
      for (int x = 0; x < R; ++x) {
        if (live(x)) {
#pragma unroll
          for (int i = 0; i < N; ++i) {
            float d = 0.f;
#pragma unroll
            for (int u = 0; u < KE; ++u) d = fmaf(q[x][i][u], f[i][u], d);
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
            if (sub == 0) sc[x][i][jj] = jj < nkr[x] ? d : -INFINITY;
          }
        }
      }
    }
  }
  __syncthreads();

  // phase 2: chunk max / exp / sum per (row, branch) (thread = key)
  float m[R * N], l[R * N];
#pragma unroll
  for (int x = 0; x < R; ++x) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float& mi = m[x * N + i];
      if (!live(x)) {
        mi = -INFINITY;
      } else if constexpr (F8) {
        // the row's K_i scale: once per (row, branch); rows >= nkr keep their -inf
        mi = -INFINITY;
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          const int j = tid + r * kThreads;
          if (j < nkr[x]) sc[x][i][j] *= ksc[r][i];
          mi = fmaxf(mi, sc[x][i][j]);
        }
      } else {
        mi = sc[x][i][tid];
#pragma unroll
        for (int r = 1; r < KPT; ++r) mi = fmaxf(mi, sc[x][i][tid + r * kThreads]);
      }
    }
  }
  block_reduce<R * N, true>(m, red);
#pragma unroll
  for (int x = 0; x < R; ++x) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float& li = l[x * N + i];
      li = 0.f;
      if (live(x)) {
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
          const int j = tid + r * kThreads;
          const float e = j < nkr[x] ? __expf(sc[x][i][j] - m[x * N + i]) : 0.f;
          if constexpr (F8) sc[x][i][j] = e * ksc[r][N];   // V's scale rides on the probability; l_i does not see it
          else sc[x][i][j] = e;
          li += e;
        }
      }
    }
  }
  block_reduce<R * N, false>(l, red);    // its barriers also publish sc

  // phase 3: acc_i = sum_j e_ij V_j (thread = VE columns of one row group)
  const int g = tid / VPR, c0 = (tid % VPR) * VE;
  const C* gv = reinterpret_cast<const C*>(p.v.p) + h * p.v.sh + c0;
  float acc[R][N][VE];
#pragma unroll
  for (int x = 0; x < R; ++x)
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int u = 0; u < VE; ++u) acc[x][i][u] = 0.f;
  for (int jj = g; jj < nk; jj += G) {
    float f[VE];
    ldnf<C, VE>(gv + crow(p.v, jj), f);
#pragma unroll
    for (int x = 0; x < R; ++x) {
      if (live(x)) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float e = sc[x][i][jj];
#pragma unroll
          for (int u = 0; u < VE; ++u) acc[x][i][u] = fmaf(e, f[u], acc[x][i][u]);
        }
      }
    }
  }
  if constexpr (ROWS) __syncthreads();   // `part` lies over the scores: every thread is done with them
#pragma unroll
  for (int x = 0; x < R; ++x) {
    if (nkr[x] > 0) {                    // uniform; a chunk wholly past row x writes no partial for it
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int u = 0; u < VE; ++u) part[g][i][c0 + u] = acc[x][i][u];
      __syncthreads();
      // partial index: [b][h][s], rows: [b][h][r][s]; group pass: member bx[x]'s own one-row slot
      const int64_t row = SH ? ((int64_t)bx[x] * p.H + h) * p.S + s
                        : ROWS ? (((int64_t)b * p.H + h) * p.Tq + r0 + x) * p.S + s : ((int64_t)b * p.H + h) * p.S + s;
      float* wacc = p.ws + row * N * DV;
      for (int y = tid; y < N * DV; y += kThreads) {
        const int i = y / DV, c = y % DV;
        float a = 0.f;
#pragma unroll
        for (int gg = 0; gg < G; ++gg) a += part[gg][i][c];
        wacc[y] = a;
      }
      if constexpr (ROWS) {
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (tid == i) {
            p.ml[row * N * 2 + i * 2] = m[x * N + i];
            p.ml[row * N * 2 + i * 2 + 1] = l[x * N + i];
          }
        __syncthreads();                 // the next row reuses `part`, the next pass the scores under it
      } else {
        if (tid < N) {
          p.ml[row * N * 2 + tid * 2] = m[tid];
          p.ml[row * N * 2 + tid * 2 + 1] = l[tid];
        }
      }
    }
  }
  }
}

constexpr int kMaxPartials = 2048;            // S * N per (b, h) for the combine's LDS weights

// ROWS: one workgroup per (b, h, query row r); row r reduces the partials of its own length
// pos_b + r + 1 as the one-row combine does, and a padding row (r >= count_b) reduces none: zeros
template <class E, int N, int kChunk, bool ROWS>
__global__ __launch_bounds__(kThreads) void decode_combine_kernel(DecodeParams p) {
  __shared__ float wgt[kMaxPartials];          // [s][i] = coef_i / L_i * exp(m_is - M_i)
  __shared__ float red[kWaves * N];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int r = ROWS ? blockIdx.z : 0;
  // partial stride: the launch's S
  const int64_t row0 = ROWS ? (((int64_t)b * p.H + h) * p.Tq + r) * p.S : ((int64_t)b * p.H + h) * p.S;
  int len;
  if constexpr (ROWS) {
    const RowSpan sp = row_span(p, b);
    len = r < sp.cnt ? sp.pos + r + 1 : 0;
  } else {
    len = clamp_len(p, b);
  }
  const int S = min((len + kChunk - 1) / kChunk, p.S);  // chunks written this call
  const float* ml = p.ml + row0 * N * 2;
  float M[N], Ls[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    M[i] = -INFINITY;
    for (int s = tid; s < S; s += kThreads) M[i] = fmaxf(M[i], ml[s * N * 2 + i * 2]);
  }
  block_reduce<N, true>(M, red);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    Ls[i] = 0.f;
    for (int s = tid; s < S; s += kThreads) {
      const float e = __expf(ml[s * N * 2 + i * 2] - M[i]);
      wgt[s * N + i] = e;
      Ls[i] += ml[s * N * 2 + i * 2 + 1] * e;
    }
  }
  block_reduce<N, false>(Ls, red);             // barriers also publish wgt
  E* go = reinterpret_cast<E*>(p.o.p) + b * p.o.sb + h * p.o.sh + (ROWS ? r * p.o.st : 0);
  const float* a = p.ws + row0 * N * p.DV;
  float c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = p.coef[h * N + i] / Ls[i];
  for (int col = tid; col < p.DV; col += kThreads) {
    float o = 0.f;
#pragma unroll 4
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int i = 0; i < N; ++i) o = fmaf(c[i] * wgt[s * N + i], a[((int64_t)s * N + i) * p.DV + col], o);
    go[col] = (E)o;
  }
}

// Chunk size is chosen from the cache capacity (ldw = t_cap), not from the
// current length, so the eager path (length = pos + 1) and the graph path
// (length = t_cap, device length) launch the same chunks and reduce in the same
// order: their outputs are bitwise equal at every position.
// keys per workgroup of a split launch (0: no plan)
inline int split_chunk(const DecodeParams& p, int N) {
  constexpr int kC = DTA_DECODE_CHUNK;
  const int64_t s_cap = (p.ldw + kC - 1) / kC;
  const int chunk = s_cap * p.H * p.B >= kWideGrid ? 2 * kC : kC;
  // the combine keeps one LDS weight per (chunk, branch): gate on the chunk actually launched
  return ((int64_t)p.ldw + chunk - 1) / chunk * N > kMaxPartials ? 0 : chunk;
}

template <class E, int N, int HS, int DV, bool PG, class C, bool ROWS>
int split_launch(const DecodeParams& p0, hipStream_t st) {
  constexpr int kC = DTA_DECODE_CHUNK;
  constexpr int R = ROWS ? rows_per_pass<N, C>() : 1;
  const dim3 gc(p0.H, p0.B, ROWS ? p0.Tq : 1);
  const int chunk = split_chunk(p0, N);
  if (!chunk) return 1;
  const bool wide = chunk != kC;
  DecodeParams p = p0;
  p.S = (p0.L + chunk - 1) / chunk;            // same partial layout as C-key chunks, fewer rows used
  if (wide) {
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, 2 * kC, PG, C, R>), dim3(p.S, p.H, p.B), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL((decode_combine_kernel<E, N, 2 * kC, ROWS>), gc, dim3(kThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, kC, PG, C, R>), dim3(p.S, p.H, p.B), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL((decode_combine_kernel<E, N, kC, ROWS>), gc, dim3(kThreads), 0, st, p);
  }
  return (int)hipGetLastError();
}

template <class E, int N, bool PG, class C, bool ROWS = false>
int split_dispatch(const DecodeParams& p, hipStream_t st) {
  if (p.HS == 32 && p.DV == 64) return split_launch<E, N, 32, 64, PG, C, ROWS>(p, st);
  if (p.HS == 64 && p.DV == 128) return split_launch<E, N, 64, 128, PG, C, ROWS>(p, st);
  if (p.HS == 128 && p.DV == 256) return split_launch<E, N, 128, 256, PG, C, ROWS>(p, st);
  if (N == 1 && p.HS == 64 && p.DV == 64) return split_launch<E, N, 64, 64, PG, C, ROWS>(p, st);
  if (N == 1 && p.HS == 128 && p.DV == 128) return split_launch<E, N, 128, 128, PG, C, ROWS>(p, st);
  return 1;    // no split plan: caller uses the single-pass kernel
}

// the multi-row step has the split plan only: no plan (shape, or too many partials for the
// combine's LDS weights) is unsupported, never a slower kernel
template <class E, bool PG, class C = E>
int rows_launch(const DecodeParams& p, hipStream_t st) {
  int e = 1;
  switch (p.N) {
    case 1: e = split_dispatch<E, 1, PG, C, true>(p, st); break;
    case 2: e = split_dispatch<E, 2, PG, C, true>(p, st); break;
    case 3: e = split_dispatch<E, 3, PG, C, true>(p, st); break;
    case 4: e = split_dispatch<E, 4, PG, C, true>(p, st); break;
  }
  return e == 1 ? -2 : e;
}

// A shared-prefix step: the group pass on grid (chunks, H, groups), the one-row pass on (chunks, H,
// B) and the one-row combine, on the chunk split_launch chooses for the paged call (from t_cap, H
// and the whole B) and on its partial layout.
template <class E, int N, int HS, int DV, class C>
int group_launch(const DecodeParams& p0, hipStream_t st) {
  constexpr int kC = DTA_DECODE_CHUNK;
  constexpr int R = rows_per_pass<N, C>();
  const int chunk = split_chunk(p0, N);
  if (!chunk) return 1;
  DecodeParams p = p0;
  p.S = (p0.L + chunk - 1) / chunk;
  const dim3 gg(p.S, p.H, p.sh_g), go(p.S, p.H, p.B), gc(p.H, p.B), th(kThreads);
  if (chunk != kC) {
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, 2 * kC, true, C, R, 1>), gg, th, 0, st, p);
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, 2 * kC, true, C, 1, 2>), go, th, 0, st, p);
    hipLaunchKernelGGL((decode_combine_kernel<E, N, 2 * kC, false>), gc, th, 0, st, p);
  } else {
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, kC, true, C, R, 1>), gg, th, 0, st, p);
    hipLaunchKernelGGL((decode_split_kernel<E, N, HS, DV, kC, true, C, 1, 2>), go, th, 0, st, p);
    hipLaunchKernelGGL((decode_combine_kernel<E, N, kC, false>), gc, th, 0, st, p);
  }
  return (int)hipGetLastError();
}

template <class E, int N, class C>
int group_dispatch(const DecodeParams& p, hipStream_t st) {
  if (p.HS == 32 && p.DV == 64) return group_launch<E, N, 32, 64, C>(p, st);
  if (p.HS == 64 && p.DV == 128) return group_launch<E, N, 64, 128, C>(p, st);
  if (p.HS == 128 && p.DV == 256) return group_launch<E, N, 128, 256, C>(p, st);
  if constexpr (N == 1) {
    if (p.HS == 64 && p.DV == 64) return group_launch<E, N, 64, 64, C>(p, st);
    if (p.HS == 128 && p.DV == 128) return group_launch<E, N, 128, 128, C>(p, st);
  }
  return 1;
}

template <class E, class C = E>
int groups_launch(const DecodeParams& p, hipStream_t st) {
  int e = 1;
  switch (p.N) {
    case 1: e = group_dispatch<E, 1, C>(p, st); break;
    case 2: e = group_dispatch<E, 2, C>(p, st); break;
    case 3: e = group_dispatch<E, 3, C>(p, st); break;
    case 4: e = group_dispatch<E, 4, C>(p, st); break;
  }
  return e == 1 ? -2 : e;
}

template <class E, bool PG, class C = E>
int decode_launch(const DecodeParams& p, hipStream_t st) {
  if (p.ml) {
    int e = 1;
    switch (p.N) {
      case 1: e = split_dispatch<E, 1, PG, C>(p, st); break;
      case 2: e = split_dispatch<E, 2, PG, C>(p, st); break;
      case 3: e = split_dispatch<E, 3, PG, C>(p, st); break;
      case 4: e = split_dispatch<E, 4, PG, C>(p, st); break;
    }
    if (e != 1) return e;
  }
  dim3 g(p.H, p.B);
  switch (p.N) {
    case 1: hipLaunchKernelGGL((decode_kernel<E, 1, PG, C>), g, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((decode_kernel<E, 2, PG, C>), g, dim3(kThreads), 0, st, p); break;
    case 3: hipLaunchKernelGGL((decode_kernel<E, 3, PG, C>), g, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((decode_kernel<E, 4, PG, C>), g, dim3(kThreads), 0, st, p); break;
    default: return -2;
  }
  return (int)hipGetLastError();
}

}  // namespace

// decode_shared.hip compiles this file once more with DTA_DECODE_GROUP_TU defined: the group-pass
// instantiations and their launchers only, so that the two translation units build side by side.
#ifndef DTA_DECODE_GROUP_TU
int launch_decode(int dtype, const DecodeParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H == 0) return 0;
  switch (dtype) {
    case 0: return p.pg.tbl ? decode_launch<__bf16, true>(p, st) : decode_launch<__bf16, false>(p, st);
    case 1: return p.pg.tbl ? decode_launch<_Float16, true>(p, st) : decode_launch<_Float16, false>(p, st);
    case 2: return p.pg.tbl ? decode_launch<float, true>(p, st) : decode_launch<float, false>(p, st);
  }
  return -2;
}

// q / o in dtype, the cache rows fp8 (e4m3fn) with per-(row, head) scales: paged only
int launch_decode_f8(int dtype, const DecodeParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H == 0) return 0;
  if (!p.pg.tbl || !p.kvs) return -2;
  switch (dtype) {
    case 0: return decode_launch<__bf16, true, f8e4>(p, st);
    case 1: return decode_launch<_Float16, true, f8e4>(p, st);
    case 2: return decode_launch<float, true, f8e4>(p, st);
  }
  return -2;
}

bool decode_rows_supported(int dtype, int hs, int n, int dv, int tq) {
  if (dtype < 0 || dtype > 2 || n < 1 || n > 4 || tq < 1 || tq > kMaxRows) return false;
  if ((hs == 32 && dv == 64) || (hs == 64 && dv == 128) || (hs == 128 && dv == 256)) return true;
  return n == 1 && dv == hs && (hs == 64 || hs == 128);
}

int launch_decode_rows(int dtype, const DecodeParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H == 0) return 0;
  if (!p.pos_dev || !p.ml || !decode_rows_supported(dtype, p.HS, p.N, p.DV, p.Tq)) return -2;
  switch (dtype) {
    case 0: return p.pg.tbl ? rows_launch<__bf16, true>(p, st) : rows_launch<__bf16, false>(p, st);
    case 1: return p.pg.tbl ? rows_launch<_Float16, true>(p, st) : rows_launch<_Float16, false>(p, st);
    case 2: return p.pg.tbl ? rows_launch<float, true>(p, st) : rows_launch<float, false>(p, st);
  }
  return -2;
}

int launch_decode_rows_f8(int dtype, const DecodeParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H == 0) return 0;
  if (!p.pg.tbl || !p.kvs) return -2;
  if (!p.pos_dev || !p.ml || !decode_rows_supported(dtype, p.HS, p.N, p.DV, p.Tq)) return -2;
  switch (dtype) {
    case 0: return rows_launch<__bf16, true, f8e4>(p, st);
    case 1: return rows_launch<_Float16, true, f8e4>(p, st);
    case 2: return rows_launch<float, true, f8e4>(p, st);
  }
  return -2;
}

#else   // DTA_DECODE_GROUP_TU
bool decode_shared_supported(int dtype, int hs, int n, int dv) { return decode_rows_supported(dtype, hs, n, dv, 1); }

// The one-row step of a paged batch under a shared-prefix plan (without a group: the paged launch
// itself).  Split plan only: -2 without one, before anything is launched.
static int shared_launch(int dtype, bool f8, const DecodeParams& p0, hipStream_t st) {
  if ((int64_t)p0.B * p0.H == 0) return 0;
  if (!p0.pg.tbl || !p0.ml || (f8 && !p0.kvs) || !decode_shared_supported(dtype, p0.HS, p0.N, p0.DV)) return -2;
  if (!split_chunk(p0, p0.N)) return -2;
  const DecodeParams& p = p0;
  if (p.sh_g <= 0 || !p.sh_mem || !p.sh_rows) return f8 ? launch_decode_f8(dtype, p, st) : launch_decode(dtype, p, st);
  switch (dtype) {
    case 0: return f8 ? groups_launch<__bf16, f8e4>(p, st) : groups_launch<__bf16>(p, st);
    case 1: return f8 ? groups_launch<_Float16, f8e4>(p, st) : groups_launch<_Float16>(p, st);
    case 2: return f8 ? groups_launch<float, f8e4>(p, st) : groups_launch<float>(p, st);
  }
  return -2;
}

int launch_decode_shared(int dtype, const DecodeParams& p, hipStream_t st) { return shared_launch(dtype, false, p, st); }
int launch_decode_shared_f8(int dtype, const DecodeParams& p, hipStream_t st) { return shared_launch(dtype, true, p, st); }
#endif  // DTA_DECODE_GROUP_TU

}  // namespace dta
