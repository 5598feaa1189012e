// extend.hip -- multi-row differential attention over a KV cache, gfx950.
//
// Tq new query rows at absolute positions pos .. pos+Tq-1 against cache rows
// 0 .. pos+Tq-1 (append to a live cache, scoring of candidate tokens, chunked
// prefill).  For every (b, h) and row r < Tq
//   o[b, r, h, :] = sum_i coef[h][i] softmax_j(q_i[r] . K_i[j] * scale, j <= pos + r) V[j, :]
// i.e. rows pos .. of dta_attn_fwd at T = pos + Tq, inference only: nothing but O
// is written (no O_i, no LSE, no workspace).
//
// The reference's own formulation (diff_transformer.py:57-72): combine the N
// softmax maps first, then one @V.  Two passes over the key tiles:
//   pass 1  per branch the running row max m_i and row sum l_i (no accumulator)
//   merge   the workgroup's waves combine their (m_i, l_i) through LDS
//   pass 2  S_i recomputed, P = sum_i coef_i / l_i * exp2(S_i * scale * log2e - m_i),
//           packed once to the operand dtype, O^T += V^T P^T (one 32 x dv accumulator)
// so registers do not depend on N (branches are streamed through one K_i tile),
// and the partial accumulators of the waves add without a rescale (m_i is global
// before pass 2 starts).
//
// Workgroup: one tile of 32 query rows; its NW (4, 2 or 1: what fits the LDS
// budget) waves split the 32-key tiles between them (wave w takes tiles w, w+NW,
// ...), each through its own K_i / V images, so a few new rows against a long
// cache still fill the workgroup.  Matrix products are S^T = K_i Q_i^T and
// O^T += V^T P^T on 32x32 MFMA tiles (a lane owns one query column).
//
// Ragged batches (dta_attn_extend_ragged) run the same kernel: pos and the number of
// real rows come per sequence from device arrays (pos_b, count_b <= Tq), the valid
// cache rows are 0 .. pos_b + count_b - 1, the key-tile loops stop at the sequence's
// own last tile, rows count_b .. Tq-1 are written as zeros and a query tile without
// a real row exits after writing them.  The one-position launch is pos_b = pos,
// count_b = Tq: the same instructions on the same values, so equal bit for bit.
//
// Paged caches (dta_attn_extend_paged) are the PG = true instantiations: the 32 rows of
// key tile kt are rows (kt * 32) % P .. + 31 of pool page table[b][kt * 32 / P] (the page
// size P is a multiple of 32, so a tile never straddles a page).  A wave looks the page
// up once per tile, and only for tiles below its sequence's last needed one; everything
// after the address is the unpaged kernel's, so the outputs are bitwise equal.
//
// The cache tail (rows >= pos + Tq) may hold anything, NaN included: those K and V
// rows are staged as zeros (a masked probability of 0 times a NaN V row inside an
// MFMA would still be NaN), and the per-element mask j <= pos + r uses absolute
// positions (pos is not tile aligned).  Every lane runs every transposed LDS read
// (no divergence around them): tiles are padded to 32 rows, never masked by EXEC.
//
// fp8 page pools (dta_attn_extend_paged_fp8) are the C = f8e4 instantiations: the cache element
// type C is a template parameter next to E (the type of q, o and both MFMA operands), as in
// decode.hip, and with C = E every expression is the one it was.  A lane reads 16 e4m3fn bytes
// of a row and converts them while it stages the image (v_cvt_pk_f32_fp8):
//   K_i image  the bare byte values (every e4m3 value is exact in bf16, f16 and f32); the row's
//              scale k_scale[j][h][i] multiplies the fp32 S^T accumulator, once per (key, branch),
//              together with scale * log2e: the tile's 32 scales of branch i sit in a per-wave LDS
//              array next to the images and a lane reads its 16 key rows' as broadcasts
//   V image    V^ = float(byte) * v_scale[j][h] rounded once to E: the magnitude of the activations
//              the cache was written from (folded into P instead, an f16 probability times
//              amax / 448 would underflow); exact in f32
// Rows at or past the valid length are staged as zeros and their scales are never loaded (0).
#include <type_traits>

#include "dta_common.h"
#include "dta_internal.h"

namespace dta {

namespace {

constexpr int kLdsBudget = 80 * 1024;        // two workgroups per CU

struct ExtendPlan {
  int nw;                // waves per workgroup
  bool qlds;             // Q tile staged in LDS (else operand reads go to global / L1)
  int tiles_off, q_off;  // byte offsets into the dynamic LDS
  int tile_bytes;        // one wave's K_i + V images (fp8 cache: and the tile's 32 K_i scales)
  int bytes;             // total
};

// LDS: fp32 stats [nw][N][2][32] | fp32 final (m_i, coef_i / l_i) [N][2][32] |
// nw x (K_i image 32 x (HS + pad), V image 32 x (DV + pad)) | Q images [N][32][HS + pad].
// The waves' accumulators are reduced through the tile region (32 x DV fp32).
// f8: the cache rows are fp8; every wave's images are followed by fp32 [32] K_i scales.
template <class E>
bool extend_plan(int N, int HS, int DV, ExtendPlan& pl, bool f8 = false) {
  const int es = (int)sizeof(E), pad = Pad<E>::v;
  pl.tile_bytes = 32 * (HS + pad + DV + pad) * es + (f8 ? 32 * 4 : 0);
  const int qbytes = N * 32 * (HS + pad) * es;
  const int red = 32 * DV * 4;
  for (int nw = 4; nw >= 1; nw >>= 1) {
    const int head = (nw + 1) * N * 2 * 32 * 4;
    int tiles = nw * pl.tile_bytes;
    if (nw > 1 && tiles < red) tiles = red;
    if (head + tiles > kLdsBudget && nw > 1) continue;
    pl.nw = nw;
    pl.tiles_off = head;
    pl.q_off = head + tiles;
    pl.qlds = pl.q_off + qbytes <= kLdsBudget;
    pl.bytes = pl.q_off + (pl.qlds ? qbytes : 0);
    return pl.bytes <= 160 * 1024;
  }
  return false;
}

// wave-private LDS images: the wave's own writes must be visible to its other
// lanes' reads (DS operations of one wave complete in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave stages 32 rows x C columns (row j0 + r of the cache; zero when >= L)
template <class E>
__device__ __forceinline__ void stage_rows(E* img, int stride, const E* src, int64_t st, int C, int j0, int L,
                                           int lane) {
  constexpr int VEC = Ops<E>::VEC;
  const int cpr = C / VEC;
  for (int x = lane; x < 32 * cpr; x += 64) {
    const int r = x / cpr, c = (x - r * cpr) * VEC;
    const bool ok = j0 + r < L;
    stage_vec<E>(img + r * stride + c, src + (int64_t)(ok ? j0 + r : 0) * st + c, ok);
  }
}

// the fp8 pool's version: 16 bytes per lane, converted on the way.  SC: times the row's scale
// sc[(j0 + r) * sst] (the V image), rounded once to E; else the bare byte values (the K_i image)
template <class E, bool SC>
__device__ __forceinline__ void stage_rows_f8(E* img, int stride, const uint8_t* src, int64_t st, int C, int j0,
                                              int L, int lane, const float* sc, int64_t sst) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int cpr = C / 16;
  for (int x = lane; x < 32 * cpr; x += 64) {
    const int r = x / cpr, c = (x - r * cpr) * 16;
    const bool ok = j0 + r < L;
    u32x4 v = u32x4{};
    float s = 0.f;
    if (ok) {
      v = *reinterpret_cast<const u32x4*>(src + (int64_t)(j0 + r) * st + c);
      if constexpr (SC) s = sc[(int64_t)(j0 + r) * sst];
    }
    float f[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], true);
      f[4 * w] = lo[0]; f[4 * w + 1] = lo[1]; f[4 * w + 2] = hi[0]; f[4 * w + 3] = hi[1];
    }
    if constexpr (SC) {
#pragma unroll
      for (int u = 0; u < 16; ++u) f[u] *= s;
    }
    E* dst = img + r * stride + c;
    if constexpr (sizeof(E) == 2) {
      typename Ops<E>::frag a, b;               // 16-bit images keep 16-byte aligned rows
#pragma unroll
      for (int u = 0; u < 8; ++u) { a[u] = (E)f[u]; b[u] = (E)f[8 + u]; }
      *reinterpret_cast<typename Ops<E>::frag*>(dst) = a;
      *reinterpret_cast<typename Ops<E>::frag*>(dst + 8) = b;
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) dst[u] = f[u];   // odd-stride rows
    }
  }
}

template <class E, int NDB, bool QLDS, bool PG, class C = E>
__global__ __launch_bounds__(256) void extend_kernel(ExtendParams p, int tiles_off, int q_off, int tile_bytes) {
  constexpr bool F8 = is_f8<C>;
  static_assert(!F8 || PG, "the fp8 cache is a paged cache");
  using KV = std::conditional_t<F8, uint8_t, E>;   // what a cache row holds
  using O = Ops<E>;
  using frag = typename O::frag;
  constexpr int SPB = 32 / O::KSTEP;            // k-steps of one 32-key tile in the PV product
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int hf = lane >> 5, c32 = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int N = p.N, HS = p.HS, DV = p.DV;
  const int kstr = HS + Pad<E>::v, vstr = DV + Pad<E>::v;
  const int nsq = HS / O::KSTEP, ndb = DV >> 5;
  const int r0 = blockIdx.x * 32;               // first query row of the tile
  // ragged batches: sequence b's own position and real row count, clamped so that no
  // device value can index past the cache views (one-position launch: p.pos, Tq)
  const int pos = p.pos_dev ? min(max(p.pos_dev[b], 0), p.cap - p.Tq) : p.pos;
  const int cnt = p.cnt_dev ? min(max(p.cnt_dev[b], 0), p.Tq) : p.Tq;
  if (r0 >= cnt) {                              // no real row in this tile (uniform): zeros, no cache read
    const int cpr = DV / 4;
    for (int x = tid; x < 32 * cpr; x += blockDim.x) {
      const int r = r0 + x / cpr, c = (x % cpr) * 4;
      if (r < p.Tq)
        store4<E>(reinterpret_cast<E*>(p.o.p) + b * p.o.sb + (int64_t)r * p.o.st + h * p.o.sh + c, 0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int L = pos + cnt;                      // valid cache rows of this sequence (>= 1 here)
  const int q0 = pos + r0;                      // absolute position of the tile's first row
  const int qlim = min(q0 + c32, L - 1);        // this lane's query sees keys <= qlim
  const int ntiles = (min(q0 + 32, L) + 31) >> 5;

  float* stats = reinterpret_cast<float*>(smem) + wave * N * 64;       // [i][m | l][32], this wave's
  float* fin = reinterpret_cast<float*>(smem) + nw * N * 64;           // [i][m | coef / l][32]
  E* Kw = reinterpret_cast<E*>(smem + tiles_off + wave * tile_bytes);
  E* Vw = Kw + 32 * kstr;
  [[maybe_unused]] float* Sw = reinterpret_cast<float*>(Vw + 32 * vstr);   // fp8: the staged K_i tile's scales [32]
  E* Qs = reinterpret_cast<E*>(smem + q_off);

  const E* gq = reinterpret_cast<const E*>(p.q.p) + b * p.q.sb + h * p.q.sh;
  const KV* gk = reinterpret_cast<const KV*>(p.k.p) + (PG ? 0 : b * p.k.sb) + h * p.k.sh;
  const KV* gv = reinterpret_cast<const KV*>(p.v.p) + (PG ? 0 : b * p.v.sb) + h * p.v.sh;
  // paged: key tile kt lies in pool page tile_page(kt) (view base + page * sb); stage_rows then
  // counts rows from jt, the tile's first row inside its page, with the limit L moved along
  [[maybe_unused]] const int pmask = (1 << p.pg.shift) - 1;
  auto tile_page = [&](int kt) -> int64_t {
    if constexpr (PG) return page_of(p.pg, b, kt * 32);
    else return 0;
  };
  // one wave stages branch i's K rows / the V rows of a key tile (page pg, rows jt .. jt+31, valid below Lt).
  // fp8: the scales of (page row r, head h) are kvs[pg][r][h][0 .. N], K_i's at i and V's at N
  auto stage_k = [&](int64_t pg, int i, int jt, int Lt) {
    if constexpr (F8) {
      stage_rows_f8<E, false>(Kw, kstr, gk + pg * p.k.sb + i * p.k.si, p.k.st, HS, jt, Lt, lane, nullptr, 0);
      if (lane < 32)
        Sw[lane] = jt + lane < Lt ? p.kvs[pg * p.kvs_sb + ((int64_t)(jt + lane) * p.H + h) * (N + 1) + i] : 0.f;
    } else {
      stage_rows<E>(Kw, kstr, gk + pg * p.k.sb + i * p.k.si, p.k.st, HS, jt, Lt, lane);
    }
  };
  auto stage_v = [&](int64_t pg, int jt, int Lt) {
    if constexpr (F8)
      stage_rows_f8<E, true>(Vw, vstr, gv + pg * p.v.sb, p.v.st, DV, jt, Lt, lane,
                             p.kvs + pg * p.kvs_sb + (int64_t)h * (N + 1) + N, (int64_t)p.H * (N + 1));
    else
      stage_rows<E>(Vw, vstr, gv + pg * p.v.sb, p.v.st, DV, jt, Lt, lane);
  };

  // rows past the real ones of a partial query tile read the last real row (their result is never stored)
  if constexpr (QLDS) {
    constexpr int VEC = O::VEC;
    const int cpr = HS / VEC;
    for (int x = tid; x < N * 32 * cpr; x += blockDim.x) {
      const int ir = x / cpr, c = (x - ir * cpr) * VEC;
      const int i = ir >> 5, r = ir & 31;
      stage_vec<E>(Qs + ir * kstr + c, gq + (int64_t)min(r0 + r, cnt - 1) * p.q.st + i * p.q.si + c, true);
    }
  }
  for (int i = 0; i < N; ++i) {
    stats[i * 64 + c32] = -INFINITY;
    stats[i * 64 + 32 + c32] = 0.f;
  }
  __syncthreads();

  auto qrow = [&](int i) -> const E* {
    if constexpr (QLDS) return Qs + (i * 32 + c32) * kstr;
    else return gq + (int64_t)min(r0 + c32, cnt - 1) * p.q.st + i * p.q.si;
  };
  // S^T (keys x queries) of branch i against the staged K_i image, in log2 units;
  // masked: key kt*32 + rowof(r, hf) above this lane's query position -> -inf.
  // fp8: register r is key row rowof(r, hf), whose scale (0 at and past the valid length, where the
  // mask holds anyway) rides on scale * log2e
  auto scores = [&](int i, int kt, bool masked) -> f32x16 {
    const E* kr = Kw + c32 * kstr;
    const E* qr = qrow(i);
    f32x16 sa = {};
#pragma unroll 4
    for (int s = 0; s < nsq; ++s) sa = O::mma(O::row(kr, s, hf), O::row(qr, s, hf), sa);
    const int lim = qlim - kt * 32 - 4 * hf;
    [[maybe_unused]] f32x4 ks[4];
    if constexpr (F8) {
#pragma unroll
      for (int g = 0; g < 4; ++g) ks[g] = *reinterpret_cast<const f32x4*>(Sw + 8 * g + 4 * hf);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float t;
      if constexpr (F8) t = sa[r] * (p.sl2 * ks[r >> 2][r & 3]);
      else t = sa[r] * p.sl2;
      sa[r] = (masked && (r & 3) + 8 * (r >> 2) > lim) ? -INFINITY : t;
    }
    return sa;
  };

  // ---- pass 1: running (m_i, l_i) of this wave's key tiles
  for (int kt = wave; kt < ntiles; kt += nw) {
    const bool masked = kt * 32 + 31 > q0;
    const int64_t pg = tile_page(kt);
    const int jt = PG ? (kt * 32) & pmask : kt * 32, Lt = PG ? L - kt * 32 + jt : L;
    for (int i = 0; i < N; ++i) {
      wave_sync();                                 // the previous image's reads are done
      stage_k(pg, i, jt, Lt);
      wave_sync();
      const f32x16 sa = scores(i, kt, masked);
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sa[r]);
      mt = wave_max_halves(mt);
      const float mo = stats[i * 64 + c32], lo = stats[i * 64 + 32 + c32];
      const float mn = fmaxf(mo, mt);
      const float ms = mn == -INFINITY ? 0.f : mn;  // a tile wholly above the row: no NaN from inf - inf
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) sum += exp2_fast(sa[r] - ms);
      sum = wave_sum_halves(sum);
      stats[i * 64 + c32] = mn;
      stats[i * 64 + 32 + c32] = fmaf(lo, exp2_fast(mo - ms), sum);
    }
  }
  __syncthreads();

  // ---- merge: global m_i and coef_i / l_i per query row (tile 0 holds key 0, so m_i is finite)
  {
    const float* all = reinterpret_cast<const float*>(smem);
    for (int x = tid; x < N * 32; x += blockDim.x) {
      const int i = x >> 5, q = x & 31;
      float M = -INFINITY;
      for (int w = 0; w < nw; ++w) M = fmaxf(M, all[(w * N + i) * 64 + q]);
      float l = 0.f;
      for (int w = 0; w < nw; ++w)
        l = fmaf(all[(w * N + i) * 64 + 32 + q], exp2_fast(all[(w * N + i) * 64 + q] - M), l);
      fin[i * 64 + q] = M;
      fin[i * 64 + 32 + q] = p.coef[h * N + i] / l;
    }
  }
  __syncthreads();

  // ---- pass 2: combined probabilities, one PV product
  f32x16 acc[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d) acc[d] = f32x16{};
  for (int kt = wave; kt < ntiles; kt += nw) {
    const bool masked = kt * 32 + 31 > q0;
    const int64_t pg = tile_page(kt);
    const int jt = PG ? (kt * 32) & pmask : kt * 32, Lt = PG ? L - kt * 32 + jt : L;
    wave_sync();
    stage_v(pg, jt, Lt);
    f32x16 pt = {};
    for (int i = 0; i < N; ++i) {
      wave_sync();
      stage_k(pg, i, jt, Lt);
      wave_sync();
      const f32x16 sa = scores(i, kt, masked);
      const float mi = fin[i * 64 + c32], ci = fin[i * 64 + 32 + c32];
#pragma unroll
      for (int r = 0; r < 16; ++r) pt[r] = fmaf(ci, exp2_fast(sa[r] - mi), pt[r]);
    }
    frag pf[SPB];
    if constexpr (SPB == 2) {
      pf[0] = O::template pack<0>(pt);
      pf[1] = O::template pack<1>(pt);
    } else {
#pragma unroll
      for (int s = 0; s < SPB; ++s) pf[s] = pt[s];
    }
    wave_sync();                                   // V image (staged before the branch loop)
#pragma unroll
    for (int d = 0; d < NDB; ++d)
      if (d < ndb) {                               // uniform: every lane runs the transposed reads
#pragma unroll
        for (int s = 0; s < SPB; ++s) acc[d] = O::mma(O::tr_perm(Vw + d * 32, vstr, s, hf, lane), pf[s], acc[d]);
      }
  }

  // ---- the waves' partial accumulators add up in wave 0 (through the tile region)
  float* red = reinterpret_cast<float*>(smem + tiles_off);
  for (int w = 1; w < nw; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int d = 0; d < NDB; ++d)
        if (d < ndb)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(d * 16 + r) * 64 + lane] = acc[d][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int d = 0; d < NDB; ++d)
        if (d < ndb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[d][r] += red[(d * 16 + r) * 64 + lane];
    }
  }
  // O^T: registers 4g..4g+3 of block d = columns 32d + 8g + 4hf .. +3 of query row c32
  // (rows cnt .. Tq-1 of a ragged batch are padding: zeros)
  if (wave == 0 && r0 + c32 < p.Tq) {
    E* go = reinterpret_cast<E*>(p.o.p) + b * p.o.sb + (int64_t)(r0 + c32) * p.o.st + h * p.o.sh;
    const bool real = r0 + c32 < cnt;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
      if (d < ndb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          store4<E>(go + d * 32 + 8 * g + 4 * hf, real ? acc[d][4 * g] : 0.f, real ? acc[d][4 * g + 1] : 0.f,
                    real ? acc[d][4 * g + 2] : 0.f, real ? acc[d][4 * g + 3] : 0.f);
  }
}

template <class E, int NDB, bool QLDS, bool PG, class C>
int extend_go(const ExtendParams& p, const ExtendPlan& pl, hipStream_t st) {
  auto kern = extend_kernel<E, NDB, QLDS, PG, C>;
  // more than the default dynamic LDS limit: raised once per instantiation
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr != hipSuccess) return (int)attr;
  const dim3 grid((p.Tq + 31) / 32, p.H, p.B);
  hipLaunchKernelGGL(kern, grid, dim3(pl.nw * 64), pl.bytes, st, p, pl.tiles_off, pl.q_off, pl.tile_bytes);
  return (int)hipGetLastError();
}

template <class E, bool PG, class C = E>
int extend_launch(const ExtendParams& p, hipStream_t st) {
  ExtendPlan pl;
  if (!extend_plan<E>(p.N, p.HS, p.DV, pl, is_f8<C>)) return -2;
  const int ndb = p.DV / 32;
  if (pl.qlds) {
    if (ndb <= 2) return extend_go<E, 2, true, PG, C>(p, pl, st);
    if (ndb <= 4) return extend_go<E, 4, true, PG, C>(p, pl, st);
    return extend_go<E, 8, true, PG, C>(p, pl, st);
  }
  if (ndb <= 2) return extend_go<E, 2, false, PG, C>(p, pl, st);
  if (ndb <= 4) return extend_go<E, 4, false, PG, C>(p, pl, st);
  return extend_go<E, 8, false, PG, C>(p, pl, st);
}

}  // namespace

bool extend_supported(int dtype, int hs, int n, int dv) {
  if (dtype < 0 || dtype > 2) return false;
  if (hs < 16 || hs > 128 || hs % 16 || dv < 32 || dv > 256 || dv % 32 || n < 1 || n > 8) return false;
  ExtendPlan pl;
  return dtype == 2 ? extend_plan<float>(n, hs, dv, pl) : extend_plan<__bf16>(n, hs, dv, pl);
}

int launch_extend(int dtype, const ExtendParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H * p.Tq == 0) return 0;
  if (!extend_supported(dtype, p.HS, p.N, p.DV)) return -2;
  switch (dtype) {
    case 0: return p.pg.tbl ? extend_launch<__bf16, true>(p, st) : extend_launch<__bf16, false>(p, st);
    case 1: return p.pg.tbl ? extend_launch<_Float16, true>(p, st) : extend_launch<_Float16, false>(p, st);
    case 2: return p.pg.tbl ? extend_launch<float, true>(p, st) : extend_launch<float, false>(p, st);
  }
  return -2;
}

// q / o in dtype, the cache rows fp8 (e4m3fn) with per-(row, head) scales: paged only.  The shapes
// both the extend plans and the quantising write (dta_kv_quant_rows) take.
bool extend_f8_supported(int dtype, int hs, int n, int dv) {
  if (dtype < 0 || dtype > 2) return false;
  if (hs < 16 || hs > 128 || hs % 16 || dv < 32 || dv > 256 || dv % 32 || n < 1 || n > 4) return false;
  ExtendPlan pl;
  return dtype == 2 ? extend_plan<float>(n, hs, dv, pl, true) : extend_plan<__bf16>(n, hs, dv, pl, true);
}

int launch_extend_f8(int dtype, const ExtendParams& p, hipStream_t st) {
  if ((int64_t)p.B * p.H * p.Tq == 0) return 0;
  if (!p.pg.tbl || !p.kvs || !extend_f8_supported(dtype, p.HS, p.N, p.DV)) return -2;
  switch (dtype) {
    case 0: return extend_launch<__bf16, true, f8e4>(p, st);
    case 1: return extend_launch<_Float16, true, f8e4>(p, st);
    case 2: return extend_launch<float, true, f8e4>(p, st);
  }
  return -2;
}

}  // namespace dta
