// gls_band_lu.hip -- kernels of the band-storage FP32 LU (gls_band_lu.hpp): the CSR -> panel scatter, the forward /
// backward substitution on the panels, and the FP64 CSR residual with a pinned unknown.
//
// Layout (gls_band_layout.hpp): block column k of width nb is one 3 nb x nb column-major panel [U_{k-1}; D_k; L_k].
// The substitution is the dense factor's kernel on the panels' addressing (gls_lu_step.hpp, LuBand). All offsets are
// 64-bit (3 n nb floats pass 2^31).
#include "gls_band_lu.hpp"
#include "gls_lu_step.hpp"

#include <algorithm>

namespace gls {

namespace {

// one thread per CSR row: each entry has one destination (no atomics). Row pin writes its diagonal 1 alone; the
// other rows skip column pin (the panels were zeroed)
__global__ void k_band_scatter(float *__restrict__ P, int64_t n, int64_t nb, const int64_t *__restrict__ rowp,
                               const int32_t *__restrict__ col, const double *__restrict__ val, int64_t pin) {
  const int64_t lda = 3 * nb;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    if (r == pin) {
      P[r * lda + r - (r / nb) * nb + nb] = 1.f;
      continue;
    }
    for (int64_t e = rowp[r]; e < rowp[r + 1]; ++e) {
      const int64_t c = col[e];
      const int64_t lr = r - (c / nb) * nb + nb;  // the row inside column c's 3 nb floats
      if (c == pin || c < 0 || c >= n || lr < 0 || lr >= lda) continue;
      P[c * lda + lr] = (float)val[e];
    }
  }
}

// 8 lanes per row, each a strided part of the row, folded by a xor tree: a fixed order. out may be b (an element is
// read and written by the same lane)
constexpr int kSpL = 8;
__global__ void k_band_csr_residual(double *out, const double *b, const double *__restrict__ x,
                                    const int64_t *__restrict__ rowp, const int32_t *__restrict__ col,
                                    const double *__restrict__ val, int64_t n, int64_t pin) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t r = t / kSpL;
  const int l = (int)(t % kSpL);
  double s = 0.0;
  if (r < n && r != pin)
    for (int64_t e = rowp[r] + l; e < rowp[r + 1]; e += kSpL) {
      const int32_t c = col[e];
      if (c != pin) s += val[e] * x[c];
    }
#pragma unroll
  for (int o = kSpL / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kSpL);
  if (r < n && l == 0) out[r] = b[r] - (r == pin ? x[r] : s);
}

}  // namespace

hipError_t band_scatter_csr(float *P, int64_t n, int64_t nb, int64_t n_floats, const int64_t *rowp, const int32_t *col,
                            const double *val, int64_t pin, hipStream_t s) {
  if (n <= 0 || nb <= 0 || n_floats != 3 * n * nb) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(P, 0, sizeof(float) * (size_t)n_floats, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_band_scatter, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, s, P, n, nb,
                     rowp, col, val, pin);
  return hipGetLastError();
}

int band_lu_solve_launches(int64_t n) { return n <= 0 ? 0 : (int)(2 * ((n + kLuB - 1) / kLuB)); }

hipError_t band_lu_solve_f32(const float *P, int64_t n, int64_t nb, int64_t bl, int64_t bu, float *x, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  // the grid of a step follows bl / bu: beyond nb a row block would lie outside its column's panel
  if (n >= INT32_MAX || nb < kLuB || nb % kLuB != 0 || 3 * nb > INT32_MAX || bl < 0 || bu < 0 || bl > nb || bu > nb)
    return hipErrorInvalidValue;
  const LuBand ad{(int)n, (int)nb};
  if (n % 4 == 0 && reinterpret_cast<uintptr_t>(P) % 16 == 0) lu_solve_steps<true>(P, ad, x, s, (int)bl, (int)bu);
  else lu_solve_steps<false>(P, ad, x, s, (int)bl, (int)bu);
  return hipGetLastError();
}

hipError_t band_csr_residual(double *out, const double *b, const double *x, const int64_t *rowp, const int32_t *col,
                             const double *val, int64_t n, int64_t pin, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_band_csr_residual, dim3((unsigned)((n * kSpL + 255) / 256)), dim3(256), 0, s, out, b, x, rowp, col,
                     val, n, pin);
  return hipGetLastError();
}

}  // namespace gls
