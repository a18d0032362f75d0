// gls_band_layout.hpp -- internal, host only (no HIP): the block-tridiagonal ("band") storage of the coarsest level's
// FP32 LU (gls_band_lu.hpp) -- its sizes, its 64-bit offsets, and the bandwidth scan of a CSR pattern.
//
// The n x n matrix with lower / upper bandwidths bl / bu is cut into block columns nb >= max(bl, bu, 1) wide. Block
// column k is one contiguous 3 nb x nb column-major panel [U_{k-1}; D_k; L_k] (lda = 3 nb): the rows of block rows
// k - 1, k and k + 1. Column j of the matrix therefore starts at float j * 3 nb, and its row i sits
// i - (j / nb) nb + nb floats further. The last block column is partial (n - k nb columns); the first panel's U part,
// the last panel's L part and the rows past n are never written after the zero fill. 3 n nb floats in all, which
// passes 2^31 at the sizes this is for: every offset is an int64_t.
#pragma once
#include <cstdint>

namespace gls_impl {

constexpr int64_t kBandSub = 128;  // the substitution's sub-block (kLuB): nb is a multiple of it

struct BandLayout {
  int64_t n = 0, bl = 0, bu = 0;
  int64_t nb = 0;        // block width
  int64_t n_blocks = 0;  // block columns, the last one partial
  int64_t n_floats = 0;  // 3 n nb
  int64_t lda() const { return 3 * nb; }
  int64_t panel(int64_t k) const { return k * nb * lda(); }  // block column k's first float
  int64_t at(int64_t i, int64_t j) const { return j * lda() + i - (j / nb) * nb + nb; }  // entry (i, j) inside the band
};

// block = 0: nb = max(bl, bu) rounded up to a multiple of 256, at least 512 (few wide rocSOLVER calls); block > 0: nb =
// block, a multiple of 128 that covers the band. Returns nullptr, or what is wrong with the arguments
inline const char *band_layout(int64_t n, int64_t bl, int64_t bu, int64_t block, BandLayout *L) {
  if (n <= 0 || n >= INT32_MAX) return "n must be in 1 .. 2^31 - 2";
  if (bl < 0 || bu < 0 || bl >= n || bu >= n) return "bandwidths must be in 0 .. n - 1";
  const int64_t w = bl > bu ? bl : bu;
  int64_t nb = ((w + 255) / 256) * 256;
  if (nb < 512) nb = 512;
  if (block != 0) {
    if (block < kBandSub || block % kBandSub != 0) return "block must be 0 (automatic) or a multiple of 128";
    if (block < w) return "block is narrower than the band";
    nb = block;
  }
  if (3 * nb > INT32_MAX) return "band too wide for rocBLAS's 32-bit leading dimension";
  L->n = n, L->bl = bl, L->bu = bu, L->nb = nb;
  L->n_blocks = (n + nb - 1) / nb;
  L->n_floats = 3 * n * nb;
  return nullptr;
}

// the bandwidths of a CSR pattern (bl = max r - c, bu = max c - r); nullptr, or what is wrong with the pattern
inline const char *csr_bandwidths(int64_t n, const int64_t *rowp, const int32_t *col, int64_t *bl, int64_t *bu) {
  if (n <= 0 || !rowp || !col || rowp[0] != 0) return "CSR: n >= 1, arrays, rowp[0] = 0";
  int64_t l = 0, u = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (rowp[r + 1] < rowp[r]) return "CSR: row offsets not monotone";
    for (int64_t e = rowp[r]; e < rowp[r + 1]; ++e) {
      const int64_t c = col[e];
      if (c < 0 || c >= n) return "CSR: column out of range";
      if (r - c > l) l = r - c;
      if (c - r > u) u = c - r;
    }
  }
  *bl = l, *bu = u;
  return nullptr;
}

}  // namespace gls_impl
