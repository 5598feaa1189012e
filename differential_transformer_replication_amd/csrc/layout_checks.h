// layout_checks.h -- which dta_tensor layouts the LDS-DMA staging of the attention kernels
// may serve.  Host code only, plain C++ (no HIP): attn_kernels.h decides with these per
// launch, and a stand-alone program can call them (tests/test_layout_checks_cpu.py).
//
// The 16-bit plans with head size >= 32 stage a tile's rows (K_i / V in the query-major
// kernels, Q_i / dO in the key-major one) by buffer_load ... lds through one descriptor
// per tile and tensor:
//   base   = the tile's first row of branch 0, a 64-bit address;
//   bound  = rows * st * es bytes, rows = T - first row (reads at or past it give zeros:
//            that is how rows >= T are masked);
//   offset = r * st * es + i * si * es + c * 16, each term and the sum in 32 bits.
// Row r < rows of branch i is therefore read whole iff r*st + i*si + width <= rows*st for
// every r, i, that is iff every branch of a row lies inside that row's stride,
//   (n - 1) * si + width <= st,
// and bound and offsets are what they should be iff the largest of them fits the
// descriptor's signed 32-bit record count, T * st * es < 2^31.  A layout that misses either
// (branch-outer Q / K with si >= T * st, a zero row stride, a view with rows 2^25 elements
// apart) is no error: the launch takes the same kernel with the tiles staged by 64-bit
// addresses instead (template argument SRD = false), which accepts any strides the C ABI
// admits and computes the same values.
#pragma once
#include <stdint.h>

namespace dta {

// rows [0, T) of n branches of `width` elements of `es` bytes at element strides st (row)
// and si (branch): whether one descriptor per tile reads them right.  No product here
// overflows, whatever strides the caller passes.
inline bool dma_rows_ok(int64_t T, int64_t st, int64_t si, int n, int width, int es) {
  if (T <= 0) return true;
  if (st <= 0 || si < 0 || width > st) return false;
  if (n > 1 && si > (st - width) / (n - 1)) return false;       // (n - 1) * si + width <= st
  return st <= ((1ll << 31) - 1) / (T * es);                    // T * st * es < 2^31
}

// the fp32 row vectors (LSE, delta: [i][b][h][t], contiguous) the key-major ring also stages
inline bool dma_rowvecs_ok(int64_t n, int64_t B, int64_t H, int64_t T) {
  const int64_t lim = ((1ll << 31) - 1) / 4;
  if (n <= 0 || B <= 0 || H <= 0 || T <= 0) return true;
  if (n > lim || B > lim || H > lim || T > lim) return false;
  if (n * B > lim || n * B * H > lim) return false;
  return n * B * H * T <= lim;                                  // n * B * H * T * 4 < 2^31
}

}  // namespace dta
