// gls_band_lu.hpp -- internal: an unpivoted FP32 LU of a banded matrix in block-tridiagonal storage
// (gls_band_layout.hpp), filled from an FP64 CSR, for coarsest multigrid levels whose n x n array does not fit.
// BandLU owns the panels and the solve's scratch vectors; the CSR, the rocBLAS handle and the streams are its caller's
// (CoarseSolve in gls_mg_coarse.cpp; the stand-alone gls_band_lu_* handle in gls_band_lu.cpp). Nothing here allocates
// n^2 of anything: the factor check and the refinement step multiply by the FP64 CSR.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include <rocblas/rocblas.h>

#include "gls_band_layout.hpp"
#include "gls_devbuf.hpp"

namespace gls {  // kernels (gls_band_lu.hip)
// P (L.n_floats floats, zeroed here) <- the CSR's values rounded to FP32 in the band layout; row and column pin
// (pin >= 0) -> identity. Every entry must lie inside the band (|r - c| <= nb); one outside it is skipped
hipError_t band_scatter_csr(float *P, int64_t n, int64_t nb, int64_t n_floats, const int64_t *rowp, const int32_t *col,
                            const double *val, int64_t pin, hipStream_t s);
// x <- (LU)^-1 x for the unpivoted factor in the panels; 2 ceil(n / 128) launches, sums in a fixed order
hipError_t band_lu_solve_f32(const float *P, int64_t n, int64_t nb, int64_t bl, int64_t bu, float *x, hipStream_t s);
// out = b - A x for the CSR with row and column pin replaced by identity (FP64; out != x)
hipError_t band_csr_residual(double *out, const double *b, const double *x, const int64_t *rowp, const int32_t *col,
                             const double *val, int64_t n, int64_t pin, hipStream_t s);
int band_lu_solve_launches(int64_t n);
}  // namespace gls

namespace gls_impl {

struct BandLU {
  BandLayout L;
  int64_t pin = -1;
  const int64_t *rowp = nullptr;  // the FP64 CSR the panels were filled from (device, the caller's)
  const int32_t *col = nullptr;
  const double *val = nullptr;
  DevBuf<float> panels, x32;
  DevBuf<double> work;  // 2 n: the residual and the first solve's x (check, refinement)
  DevBuf<double> rel;   // |A x - 1| of the check (device pointer mode)
  DevBuf<int> info;
  size_t bytes() const { return sizeof(float) * (size_t)L.n_floats; }

  int init(const BandLayout &layout);  // allocations only
  // the panels from the CSR on s (the pointers are kept for check / refinement: they stay valid and unchanged until
  // the next fill)
  int fill(hipStream_t s, const int64_t *rowp_, const int32_t *col_, const double *val_, int64_t pin_);
  // the block sequence getrf_npvt / trsm / gemm on h's stream, then the check |A x - 1| / |1| queued there (rel);
  // rocSOLVER returns when each block is done, so CoarseSolve calls this from its worker thread. 0, or the failing
  // step's number (3 factorization, 4 check)
  int factor(rocblas_handle h, hipStream_t s);
  // after the stream has drained: *check = |A x - 1| / |1| (INFINITY for a zero pivot in the last block or a
  // non-finite value)
  int read_check(hipStream_t s, double *check);
  // x = A^-1 b (FP64 in and out, b == x allowed), refine: one step x += LU^-1 (b - A x) against the FP64 CSR
  int solve(hipStream_t s, const double *b, double *x, bool refine);
};

}  // namespace gls_impl
