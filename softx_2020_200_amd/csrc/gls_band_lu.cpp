// gls_band_lu.cpp -- the band-storage FP32 LU (gls_band_lu.hpp): allocation, the rocSOLVER / rocBLAS block sequence
// on the panels, its check and the solve; and the stand-alone gls_band_lu_* entry points (tests and tools).
#include "gls_band_lu.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "gls_launch.hpp"

namespace gls_impl {
namespace {
constexpr rocblas_status kOk = rocblas_status_success;
}

int BandLU::init(const BandLayout &layout) {
  L = layout;
  GLS_TRY(panels.alloc((size_t)L.n_floats));
  GLS_TRY(x32.alloc((size_t)L.n));
  GLS_TRY(work.alloc((size_t)(2 * L.n)));
  GLS_TRY(rel.alloc(1));
  GLS_TRY(info.alloc(1));
  return GLS_OK;
}

int BandLU::fill(hipStream_t s, const int64_t *rowp_, const int32_t *col_, const double *val_, int64_t pin_) {
  if (pin_ >= L.n) return set_err(GLS_EINVAL, "band LU: pinned unknown %lld outside the matrix", (long long)pin_);
  rowp = rowp_, col = col_, val = val_, pin = pin_ < 0 ? -1 : pin_;
  HIP_TRY(gls::band_scatter_csr(panels.p, L.n, L.nb, L.n_floats, rowp, col, val, pin, s));
  return GLS_OK;
}

// Right-looking by block columns, start_f32's sequence with the panels' base pointers: the block's panel [D_k; L_k]
// down to the lower band, its rows of U (the U part of panel k + 1) to the upper band, the trailing update of
// D_{k+1}'s corner. Without pivoting nothing outside the band fills.
int BandLU::factor(rocblas_handle h, hipStream_t s) {
  const int64_t n = L.n, nb = L.nb, bl = L.bl, bu = L.bu;
  const rocblas_int lda = (rocblas_int)L.lda();
  const float fone = 1.0f, fmone = -1.0f;
  if (rocblas_set_stream(h, s) != kOk) return 2;
  for (int64_t k = 0; k < L.n_blocks; ++k) {
    const int64_t k0 = k * nb, kb = std::min(nb, n - k0), mr = std::min(n - k0, kb + bl);
    const int64_t nc = std::min(n - k0 - kb, bu);
    float *A11 = panels.p + L.panel(k) + nb;         // D_k
    float *A12 = nc > 0 ? panels.p + L.panel(k + 1) : nullptr;  // U_k: block row k of panel k + 1
    if (rocsolver_sgetrf_npvt(h, (rocblas_int)mr, (rocblas_int)kb, A11, lda, info.p) != kOk) return 3;
    if (nc > 0 && rocblas_strsm(h, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_unit,
                                (rocblas_int)kb, (rocblas_int)nc, &fone, A11, lda, A12, lda) != kOk)
      return 3;
    if (nc > 0 && mr > kb &&
        rocblas_sgemm(h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)(mr - kb), (rocblas_int)nc,
                      (rocblas_int)kb, &fmone, A11 + kb, lda, A12, lda, &fone, A12 + nb, lda) != kOk)
      return 3;
  }
  // the check: x = LU^-1 b for b = 1 (pinned row 0), |b - A x| against the FP64 CSR
  double *b = work.p, *x = work.p + n;
  bool good = gls::vec_fill(b, n, 1.0, s) == hipSuccess;
  if (good && pin >= 0) good = hipMemsetAsync(b + pin, 0, sizeof(double), s) == hipSuccess;
  good = good && gls::vec_to_f32(b, x32.p, n, s) == hipSuccess &&
         gls::band_lu_solve_f32(panels.p, n, nb, bl, bu, x32.p, s) == hipSuccess &&
         gls::vec_from_f32(x32.p, x, n, s) == hipSuccess &&
         gls::band_csr_residual(b, b, x, rowp, col, val, n, pin, s) == hipSuccess &&
         rocblas_set_pointer_mode(h, rocblas_pointer_mode_device) == kOk &&
         rocblas_dnrm2(h, (rocblas_int)n, b, 1, rel.p) == kOk;
  (void)rocblas_set_pointer_mode(h, rocblas_pointer_mode_host);
  return good ? 0 : 4;
}

int BandLU::read_check(hipStream_t s, double *check) {
  int inf = -1;
  double rn = INFINITY;
  HIP_TRY(hipMemcpyAsync(&inf, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&rn, rel.p, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // info is the LAST block's (every getrf_npvt call overwrites it): it only screens; the residual decides
  const double r = rn / std::sqrt((double)L.n);
  *check = inf == 0 && std::isfinite(r) ? r : INFINITY;
  return GLS_OK;
}

int BandLU::solve(hipStream_t s, const double *b, double *x, bool refine) {
  const int64_t n = L.n;
  HIP_TRY(gls::vec_to_f32(b, x32.p, n, s));
  HIP_TRY(gls::band_lu_solve_f32(panels.p, n, L.nb, L.bl, L.bu, x32.p, s));
  if (!refine) {
    HIP_TRY(gls::vec_from_f32(x32.p, x, n, s));
    return GLS_OK;
  }
  double *r = work.p, *x0 = work.p + n;  // r = b - A x0 (the pinned FP64 CSR), x = x0 + LU^-1 r
  HIP_TRY(gls::vec_from_f32(x32.p, x0, n, s));
  HIP_TRY(gls::band_csr_residual(r, b, x0, rowp, col, val, n, pin, s));
  HIP_TRY(gls::vec_to_f32(r, x32.p, n, s));
  HIP_TRY(gls::band_lu_solve_f32(panels.p, n, L.nb, L.bl, L.bu, x32.p, s));
  HIP_TRY(gls::vec_from_f32(x32.p, x, n, s));
  HIP_TRY(gls::vec_axpy(x, 1.0, x0, n, s));
  return GLS_OK;
}

}  // namespace gls_impl

using namespace gls_impl;

struct gls_band_lu {
  BandLU lu;
  DevBuf<int64_t> rowp;
  DevBuf<int32_t> col;
  DevBuf<double> val;
  rocblas_handle blas = nullptr;
  double check = INFINITY;
  ~gls_band_lu() {
    (void)hipDeviceSynchronize();
    if (blas) rocblas_destroy_handle(blas);
  }
};

extern "C" {

int gls_band_lu_layout(int64_t n, int64_t bl, int64_t bu, int64_t block, int64_t *nb, int64_t *n_blocks, int64_t *n_floats) {
  BandLayout L;
  if (const char *why = band_layout(n, bl, bu, block, &L)) return set_err(GLS_EINVAL, "gls_band_lu_layout: %s", why);
  if (nb) *nb = L.nb;
  if (n_blocks) *n_blocks = L.n_blocks;
  if (n_floats) *n_floats = L.n_floats;
  return GLS_OK;
}

int gls_band_lu_create(int64_t n, const int64_t *rowp, const int32_t *col, const double *val, int64_t pin, int64_t block,
                       gls_band_lu **handle) {
  if (!handle || !val) return set_err(GLS_EINVAL, "gls_band_lu_create: null argument");
  *handle = nullptr;
  int64_t bl = 0, bu = 0;
  if (const char *why = csr_bandwidths(n, rowp, col, &bl, &bu)) return set_err(GLS_EINVAL, "gls_band_lu_create: %s", why);
  BandLayout L;
  if (const char *why = band_layout(n, bl, bu, block, &L)) return set_err(GLS_EINVAL, "gls_band_lu_create: %s", why);
  if (pin >= n) return set_err(GLS_EINVAL, "gls_band_lu_create: pin %lld outside the matrix", (long long)pin);
  std::unique_ptr<gls_band_lu> H(new gls_band_lu);
  if (rocblas_create_handle(&H->blas) != rocblas_status_success) return set_err(GLS_EHIP, "rocblas_create_handle failed");
  const size_t nnz = (size_t)rowp[n];
  GLS_TRY(H->rowp.upload(rowp, (size_t)n + 1));
  GLS_TRY(H->col.upload(col, std::max<size_t>(nnz, 1)));
  GLS_TRY(H->val.upload(val, std::max<size_t>(nnz, 1)));
  GLS_TRY(H->lu.init(L));
  hipStream_t s = nullptr;
  GLS_TRY(H->lu.fill(s, H->rowp.p, H->col.p, H->val.p, pin));
  if (const int rc = H->lu.factor(H->blas, s)) {
    (void)hipStreamSynchronize(s);
    return set_err(GLS_EHIP, "gls_band_lu_create: the factorization failed (step %d)", rc);
  }
  GLS_TRY(H->lu.read_check(s, &H->check));
  // no pivoted fallback in band storage (an explicit inverse is n^2): a broken factor is refused here
  if (!(H->check < 0.5))
    return set_err(GLS_EINVAL, "gls_band_lu_create: unpivoted band LU failed its check, |A x - 1| / |1| = %.3e (n %lld, "
                               "bandwidths %lld / %lld)", H->check, (long long)n, (long long)bl, (long long)bu);
  *handle = H.release();
  return GLS_OK;
}

int gls_band_lu_solve(gls_band_lu *h, const double *b, double *x, int refine) {
  if (!h || !b || !x) return set_err(GLS_EINVAL, "gls_band_lu_solve: null argument");
  hipStream_t s = nullptr;
  GLS_TRY(h->lu.solve(s, b, x, refine != 0));
  if (h->lu.pin >= 0) HIP_TRY(hipMemsetAsync(x + h->lu.pin, 0, sizeof(double), s));  // pinned: no correction
  return GLS_OK;
}

int gls_band_lu_info(const gls_band_lu *h, int64_t *bl, int64_t *bu, int64_t *nb, int64_t *bytes, double *check) {
  if (!h) return set_err(GLS_EINVAL, "gls_band_lu_info: null handle");
  if (bl) *bl = h->lu.L.bl;
  if (bu) *bu = h->lu.L.bu;
  if (nb) *nb = h->lu.L.nb;
  if (bytes) *bytes = (int64_t)h->lu.bytes();
  if (check) *check = h->check;
  return GLS_OK;
}

int gls_band_lu_destroy(gls_band_lu *h) {
  delete h;
  return GLS_OK;
}

}  // extern "C"
