// gls_mg_coarse.cpp -- the multigrid's coarsest-level direct solve (gls_mg_coarse.hpp): factorization of the probed
// dense Jacobian by rocSOLVER (FP64 in place up to kDirectSmall unknowns, FP32 on a side stream above) or the
// Gauss-Jordan kernel, and its application inside the V-cycle.
#include "gls_mg_coarse.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "gls_launch.hpp"

namespace gls_impl {
namespace {
constexpr rocblas_status kOk = rocblas_status_success;
bool verbose_on() { return std::getenv("GLS_MG_VERBOSE") != nullptr; }
double ms(CoarseSolve::Clock::time_point a, CoarseSolve::Clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}
// rocSOLVER's LU by precision; pivot = false: the unpivoted factorization (ipiv untouched)
rocblas_status getrf(rocblas_handle h, rocblas_int n, double *A, rocblas_int *ipiv, rocblas_int *info, bool pivot) {
  return pivot ? rocsolver_dgetrf(h, n, n, A, n, ipiv, info) : rocsolver_dgetrf_npvt(h, n, n, A, n, info);
}
rocblas_status getrf(rocblas_handle h, rocblas_int n, float *A, rocblas_int *ipiv, rocblas_int *info, bool pivot) {
  return pivot ? rocsolver_sgetrf(h, n, n, A, n, ipiv, info) : rocsolver_sgetrf_npvt(h, n, n, A, n, info);
}
rocblas_status getri(rocblas_handle h, rocblas_int n, double *A, rocblas_int *ipiv, rocblas_int *info) {
  return rocsolver_dgetri(h, n, A, n, ipiv, info);
}
rocblas_status getri(rocblas_handle h, rocblas_int n, float *A, rocblas_int *ipiv, rocblas_int *info) {
  return rocsolver_sgetri(h, n, A, n, ipiv, info);
}
}  // namespace

int CoarseSolve::init(int64_t n_) {
  n = n_;
  GLS_TRY(probe.alloc((size_t)(n * n)));
  if (n > kDirectSmall) {
    GLS_TRY(probe32.alloc((size_t)(n * n)));
    GLS_TRY(b32.alloc((size_t)n));
    GLS_TRY(x32.alloc((size_t)n));
  }
  if (std::getenv("GLS_MG_COARSE_SOLVER")) GLS_TRY(aug.alloc((size_t)(2 * n * n)));  // gj experiments
  GLS_TRY(ipiv.alloc((size_t)n));
  GLS_TRY(info.alloc(1));
  if (!blas) {
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != kOk) return set_err(GLS_EHIP, "rocblas_create_handle failed");
    blas.reset(h);
  }
  rocblas_set_pointer_mode(blas.get(), rocblas_pointer_mode_host);
  GLS_TRY(unit.alloc((size_t)n));
  GLS_TRY(status.alloc(1));
  return GLS_OK;
}

// ---- the band route: BandLU (gls_band_lu.cpp) does the work; here its place in the preparation's lifetime rules
int CoarseSolve::init_band(int64_t n_, int64_t block) {
  n = n_;
  BandLayout L;
  if (const char *why = band_layout(n, band.bl, band.bu, block, &L))
    return set_err(GLS_EINVAL, "mg: coarse band storage: %s", why);
  GLS_TRY(blu.init(L));
  GLS_TRY(tmp.alloc((size_t)n));
  if (!blas) {
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != kOk) return set_err(GLS_EHIP, "rocblas_create_handle failed");
    blas.reset(h);
  }
  rocblas_set_pointer_mode(blas.get(), rocblas_pointer_mode_host);
  band_store = true;
  if (verbose_on())
    std::printf("mg: coarse FP32 LU in band storage n=%lld bl=%lld bu=%lld nb=%lld blocks=%lld bytes=%lld\n", (long long)n,
                (long long)L.bl, (long long)L.bu, (long long)L.nb, (long long)L.n_blocks, (long long)blu.bytes());
  return GLS_OK;
}

int CoarseSolve::factor_band(hipStream_t s0, const int64_t *rowp, const int32_t *col, const double *val, int64_t pin,
                             Clock::time_point t0) {
  ok = lu = lu32 = false;
  if (pin >= n) return set_err(GLS_EINVAL, "mg: coarsest level without pressure DoFs");
  pin_dof = pin;
  banded = true;
  GLS_TRY(blu.fill(s0, rowp, col, val, band.pin));
  HIP_TRY(side.ensure());
  hipStream_t s = side.s;
  HIP_TRY(hipEventRecord(side.e0, s0));
  HIP_TRY(hipStreamWaitEvent(s, side.e0, 0));
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  side.join();
  side.rc = 0;
  auto *m = this;
  const bool verbose = verbose_on();
  side.worker = std::thread([m, s, dev, verbose]() {
    const auto h0 = Clock::now();
    int &rc = m->side.rc;
    if (hipSetDevice(dev) != hipSuccess) rc = 1;
    else rc = m->blu.factor(m->blas.get(), s);
    if (verbose) std::printf("mg: the band FP32 LU returned to its worker thread after %.2f ms\n", ms(h0, Clock::now()));
    if (!rc && hipEventRecord(m->side.e1, s) != hipSuccess) rc = 5;
  });
  pending = true;
  if (verbose) {
    (void)hipStreamSynchronize(s0);
    std::printf("mg: coarse FP32 band LU n=%lld queued on the side stream at %.2f ms\n", (long long)n, ms(t0, Clock::now()));
  }
  ok = true;
  return GLS_OK;
}

// no pivoted route in band storage (an explicit inverse is n^2): a failed check clears ok and is an error, so the
// caller prepares again and no NaN reaches a V-cycle
int CoarseSolve::finish_band() {
  double r = INFINITY;
  GLS_TRY(blu.read_check(side.s, &r));
  lu32_refine = r >= 1e-2 && r < 0.5;
  if (verbose_on())
    std::printf("mg: coarse FP32 band LU n=%lld, check |A x - 1| / |1| = %.2e%s\n", (long long)n, r,
                lu32_refine ? ", applied with one refinement step" : "");
  if (r < 0.5) return GLS_OK;
  ok = false;
  return set_err(GLS_EINVAL, "coarse band LU failed its check: |A x - 1| / |1| = %.3e (n %lld; band storage has no pivoted "
                             "route)", r, (long long)n);
}

// A <- A^-1 on s: getrf (pivoted or not), info read back, getri, info read back (one host wait each). *inf: the
// failing step's info, 0 when A holds the inverse; getri is skipped after a failed getrf
template <class T>
int CoarseSolve::invert(hipStream_t s, T *A, bool pivot, int *inf) {
  const char P = sizeof(T) == sizeof(double) ? 'd' : 's';
  if (rocblas_set_stream(blas.get(), s) != kOk || getrf(blas.get(), (rocblas_int)n, A, ipiv.p, info.p, pivot) != kOk)
    return set_err(GLS_EHIP, "rocsolver_%cgetrf failed", P);
  if (pivot) {
    npvt_ipiv_n = -1;  // getrf overwrites ipiv with its permutation
  } else if (npvt_ipiv_n != n) {  // identity permutation for getri
    std::vector<int> id((size_t)n);
    for (int64_t i = 0; i < n; ++i) id[(size_t)i] = (int)(i + 1);
    HIP_TRY(hipMemcpyAsync(ipiv.p, id.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    npvt_ipiv_n = n;
  }
  HIP_TRY(hipMemcpyAsync(inf, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t_getrf = Clock::now();
  if (*inf != 0) return GLS_OK;
  if (getri(blas.get(), (rocblas_int)n, A, ipiv.p, info.p) != kOk) return set_err(GLS_EHIP, "rocsolver_%cgetri failed", P);
  HIP_TRY(hipMemcpyAsync(inf, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GLS_OK;
}

// The explicit inverse (probe) against the pinned matrix it came from (probe_bak): y = A^-1 e, z = A y for
// e = (1, ..., 1); good = y finite and max|z - e| <= 1e-8 max(1, max|A| max|y|) (a backward-stable
// factorization leaves ~n eps there; an unpivoted LU through a tiny pivot leaves O(1) or non-finite values)
int CoarseSolve::inverse_check(hipStream_t s, bool *good) {
  *good = false;
  if (chk.n < (size_t)(2 * n)) GLS_TRY(chk.alloc((size_t)(2 * n)));
  double *y = chk.p, *z = chk.p + n;
  HIP_TRY(gls::vec_fill(unit.p, n, 1.0, s));
  const double one = 1.0, zero = 0.0;
  rocblas_int imax = 0;
  if (rocblas_set_stream(blas.get(), s) != kOk ||
      rocblas_dgemv(blas.get(), rocblas_operation_none, (rocblas_int)n, (rocblas_int)n, &one, probe.p, (rocblas_int)n, unit.p, 1,
                    &zero, y, 1) != kOk ||
      rocblas_dgemv(blas.get(), rocblas_operation_none, (rocblas_int)n, (rocblas_int)n, &one, probe_bak.p, (rocblas_int)n, y, 1,
                    &zero, z, 1) != kOk ||
      rocblas_idamax(blas.get(), (rocblas_int)(n * n), probe_bak.p, 1, &imax) != kOk)
    return set_err(GLS_EHIP, "coarse inverse check: rocBLAS failed");
  std::vector<double> h((size_t)(2 * n));
  double amax = 0.0;
  HIP_TRY(hipMemcpyAsync(h.data(), chk.p, sizeof(double) * (size_t)(2 * n), hipMemcpyDeviceToHost, s));
  if (imax > 0) HIP_TRY(hipMemcpyAsync(&amax, probe_bak.p + (imax - 1), sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double ymax = 0.0, err = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(h[(size_t)i]) || !std::isfinite(h[(size_t)(n + i)])) return GLS_OK;
    ymax = std::max(ymax, std::fabs(h[(size_t)i]));
    err = std::max(err, std::fabs(h[(size_t)(n + i)] - 1.0));
  }
  *good = err <= 1e-8 * std::max(1.0, std::fabs(amax) * ymax);
  if (verbose_on())
    std::printf("mg: coarse inverse check n=%lld max|Ay-e| %.3e max|A| %.3e max|y| %.3e -> %s\n", (long long)n, err,
                std::fabs(amax), ymax, *good ? "ok" : "FAILED");
  return GLS_OK;
}

int CoarseSolve::factor(hipStream_t s, int64_t pin, bool banded_, Clock::time_point t0) {
  const bool verbose = verbose_on();
  if (verbose) (void)hipStreamSynchronize(s);  // (the timings' phase boundary)
  const auto t1 = Clock::now();
  ok = lu = lu32 = false;
  // gj | lu | lu_npvt. Default: LU without pivoting (rocSOLVER's pivoted panel factorization is ~1 ms of
  // a Newton step at n = 500, profiles/r04_ab_env_switches.txt) with a pivoted retry when a pivot vanishes
  const char *route = std::getenv("GLS_MG_COARSE_SOLVER");
  const bool gj = n <= kDirectSmall && route && std::strncmp(route, "lu", 2) != 0;
  if (!gj && pin >= n) return set_err(GLS_EINVAL, "mg: coarsest level without pressure DoFs");
  pin_dof = pin;
  banded = banded_;
  if (n > kDirectSmall) {  // FP32 LU of the pinned matrix: unpivoted (checked), else pivoted + explicit inverse
    HIP_TRY(gls::mg_pin_dof(probe.p, n, pin_row(), s));
    HIP_TRY(gls::vec_to_f32(probe.p, probe32.p, n * n, s));
    GLS_TRY(start_f32(s));
    if (verbose) {
      (void)hipStreamSynchronize(s);
      std::printf("mg: coarse FP32 unpivoted LU n=%lld queued on the side stream at %.2f ms\n", (long long)n,
                  ms(t0, Clock::now()));
    }
    lu32 = lu32_npvt = ok = true;
    return GLS_OK;
  }
  banded = false;
  if (!gj) return factor_f64(s, route, t0, t1);  // LU: 1.5-3 ms at n = 500 vs the one-workgroup GJ's ~15
  HIP_TRY(gls::mg_dense_invert(probe.p, aug.p, (int)n, status.p, s));
  int st = -1;
  HIP_TRY(hipMemcpyAsync(&st, status.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // a couple of dependent columns (pressure gauge) are expected; many mean a broken operator
  ok = st >= 0 && st <= 4;
  if (verbose) std::printf("mg: coarse direct solve n=%lld dropped=%d ok=%d\n", (long long)n, st, (int)ok);
  return GLS_OK;
}

// FP64 LU with the pressure gauge pinned -> explicit inverse. route: GLS_MG_COARSE_SOLVER (null: unpivoted, with the
// matrix kept for a pivoted retry after a zero pivot or a failed inverse check; lu_npvt / lu: as asked, no retry)
int CoarseSolve::factor_f64(hipStream_t s, const char *route, Clock::time_point t0, Clock::time_point t1) {
  const bool verbose = verbose_on();
  bool npvt = route ? std::strcmp(route, "lu_npvt") == 0 : true;
  HIP_TRY(gls::mg_pin_dof(probe.p, n, pin_dof, s));
  if (!route) {  // keep the matrix for a pivoted retry
    if (probe_bak.n != (size_t)(n * n)) GLS_TRY(probe_bak.alloc((size_t)(n * n)));
    HIP_TRY(gls::vec_copy(probe_bak.p, probe.p, n * n, s));
  }
  auto repivot = [&]() -> int {  // the pinned matrix again, factored with partial pivoting
    npvt = false;
    HIP_TRY(gls::vec_copy(probe.p, probe_bak.p, n * n, s));
    return GLS_OK;
  };
  int inf = -1;
  GLS_TRY(invert(s, probe.p, !npvt, &inf));
  if (inf != 0 && !route) {
    if (verbose) std::printf("mg: unpivoted coarse LU hit pivot %d, retrying with pivoting\n", inf);
    GLS_TRY(repivot());
    GLS_TRY(invert(s, probe.p, true, &inf));
  }
  if (verbose) std::printf("mg: levels+probe %.2f ms, getrf %.2f ms\n", ms(t0, t1), ms(t1, t_getrf));
  // an unpivoted LU of the indefinite velocity-pressure Jacobian passes getrf with a tiny nonzero
  // pivot and can return a wildly wrong (or non-finite) inverse: check A (A^-1 e) = e and redo the
  // factorization with partial pivoting when it fails
  if (inf == 0 && npvt && !route) {
    bool good = false;
    GLS_TRY(inverse_check(s, &good));
    if (!good) {
      if (verbose) std::printf("mg: unpivoted coarse inverse failed its check, refactoring with pivoting\n");
      GLS_TRY(repivot());
      GLS_TRY(invert(s, probe.p, true, &inf));
    }
  }
  if (inf == 0) HIP_TRY(gls::mg_zero_row(probe.p, n, pin_dof, s));  // pinned unknown: zero correction
  lu = ok = inf == 0;
  if (verbose) {
    (void)hipStreamSynchronize(s);
    std::printf("mg: coarse LU n=%lld info=%d, getri done at %.2f ms\n", (long long)n, inf, ms(t0, Clock::now()));
  }
  // (getrf overwrote the matrix: the next preparation probes it again, for the Gauss-Jordan route when asked)
  if (!lu) return set_err(GLS_EINVAL, "coarse LU: zero pivot %d (set GLS_MG_COARSE_SOLVER=gj)", inf);
  return GLS_OK;
}

// the large coarsest level's FP32 factorization (kDirectSmall < n): rocSOLVER sgetrf_npvt of the pinned matrix (138 ms
// at n = 25000 against sgetrf's 410 + sgetri's ~800) and its check |A x - 1| / |1| on the side stream, ordered after
// s's probing / rounding; nothing here waits on the host
int CoarseSolve::start_f32(hipStream_t s0) {
  HIP_TRY(side.ensure());
  hipStream_t s = side.s;
  if (chk32.n != (size_t)(2 * n)) GLS_TRY(chk32.alloc((size_t)(2 * n)));
  if (rel.n != 1) GLS_TRY(rel.alloc(1));
  if (banded && tmp.n != (size_t)n) GLS_TRY(tmp.alloc((size_t)n));
  HIP_TRY(hipEventRecord(side.e0, s0));
  HIP_TRY(hipStreamWaitEvent(s, side.e0, 0));
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  side.join();
  side.rc = 0;
  auto *m = this;
  const bool verbose = verbose_on();
  const int64_t n = this->n, pin = pin_row(), bl = banded ? band.bl : -1, bu = banded ? band.bu : -1;
  side.worker = std::thread([m, s, n, pin, dev, verbose, bl, bu]() {
    const double one = 1.0, mone = -1.0;
    int &rc = m->side.rc;
    const auto h0 = Clock::now();
    // banded: right-looking by column blocks as wide as the band (rocSOLVER's calls return only when done, so few
    // wide blocks: 256-wide ones took 98 calls and longer than the dense factorization, profiles/
    // r06_ab_banded_coarse_lu.txt): the block's panel down to the lower band, its rows of U to the upper band, the
    // trailing band update; without pivoting nothing outside the band fills
    const int64_t nb = bl < 0 ? n : std::max<int64_t>(512, ((std::max(bl, bu) + 255) / 256) * 256);
    if (hipSetDevice(dev) != hipSuccess) rc = 1;
    else if (rocblas_set_stream(m->blas.get(), s) != kOk) rc = 2;
    const float fone = 1.0f, fmone = -1.0f;
    float *A = m->probe32.p;
    for (int64_t k0 = 0; k0 < n && !rc; k0 += nb) {
      const int64_t kb = std::min(nb, n - k0), mr = bl < 0 ? n - k0 : std::min(n - k0, kb + bl);
      const int64_t nc = bl < 0 ? 0 : std::min(n - k0 - kb, bu);
      float *A11 = A + k0 + k0 * n, *A12 = A + k0 + (k0 + kb) * n;
      if (rocsolver_sgetrf_npvt(m->blas.get(), (rocblas_int)mr, (rocblas_int)kb, A11, (rocblas_int)n, m->info.p) != kOk)
        rc = 3;
      else if (nc > 0 &&
               rocblas_strsm(m->blas.get(), rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_unit,
                             (rocblas_int)kb, (rocblas_int)nc, &fone, A11, (rocblas_int)n, A12, (rocblas_int)n) != kOk)
        rc = 3;
      else if (nc > 0 && mr > kb &&
               rocblas_sgemm(m->blas.get(), rocblas_operation_none, rocblas_operation_none, (rocblas_int)(mr - kb),
                             (rocblas_int)nc, (rocblas_int)kb, &fmone, A11 + kb, (rocblas_int)n, A12, (rocblas_int)n,
                             &fone, A12 + kb, (rocblas_int)n) != kOk)
        rc = 3;
    }
    if (verbose)
      std::printf("mg: the %s FP32 LU returned to its worker thread after %.2f ms\n", bl < 0 ? "dense" : "banded",
                  ms(h0, Clock::now()));
    if (!rc &&
        !(gls::vec_fill(m->chk32.p, n, 1.0, s) == hipSuccess && gls::mg_zero_row(m->chk32.p, 1, pin, s) == hipSuccess &&
          gls::vec_to_f32(m->chk32.p, m->x32.p, n, s) == hipSuccess &&
          gls::dense_lu_solve_f32(m->probe32.p, (int)n, m->x32.p, s, (int)bl, (int)bu) == hipSuccess &&
          gls::vec_from_f32(m->x32.p, m->chk32.p + n, n, s) == hipSuccess &&
          rocblas_dgemv(m->blas.get(), rocblas_operation_none, (rocblas_int)n, (rocblas_int)n, &one, m->probe.p,
                        (rocblas_int)n, m->chk32.p + n, 1, &mone, m->chk32.p, 1) == kOk &&
          rocblas_set_pointer_mode(m->blas.get(), rocblas_pointer_mode_device) == kOk &&
          rocblas_dnrm2(m->blas.get(), (rocblas_int)n, m->chk32.p, 1, m->rel.p) == kOk))
      rc = 4;
    (void)rocblas_set_pointer_mode(m->blas.get(), rocblas_pointer_mode_host);
    if (!rc && hipEventRecord(m->side.e1, s) != hipSuccess) rc = 5;
  });
  pending = true;
  return GLS_OK;
}

// A factorization that pivot growth broke (O(1) or non-finite residual) is replaced by the pivoted sgetrf + sgetri
// inverse on s. A coarse-grid correction accurate to 1 % is exact enough for the V-cycle.
int CoarseSolve::finish(hipStream_t s) {
  if (!pending) return GLS_OK;
  pending = false;
  side.join();
  (void)rocblas_set_stream(blas.get(), s);
  if (side.rc) {
    ok = lu32 = false;
    return set_err(GLS_EHIP, "coarse FP32 LU on the side stream failed (step %d)", side.rc);
  }
  if (band_store) return finish_band();
  // info is what the LAST sgetrf_npvt call left: in the banded loop every column block overwrites it (and counts
  // pivots from its own first column), so a zero pivot in an earlier block is not seen here. inf == 0 only screens;
  // the residual check below decides (a vanished pivot leaves it O(1) or non-finite)
  int inf = -1;
  double rn = INFINITY;
  HIP_TRY(hipMemcpyAsync(&inf, info.p, sizeof(int), hipMemcpyDeviceToHost, side.s));
  HIP_TRY(hipMemcpyAsync(&rn, rel.p, sizeof(double), hipMemcpyDeviceToHost, side.s));
  HIP_TRY(hipStreamSynchronize(side.s));
  const double r = inf == 0 ? rn / std::sqrt((double)n) : INFINITY;
  const bool verbose = verbose_on();
  // (below 1e-2 the correction is used as it is; up to 0.5 with one refinement step x += LU^-1 (b - A x) against the
  // FP64 matrix (an extra solve and one FP64 matrix pass per coarse solve: residual error ~ rel^2); beyond, or a
  // broken factorization, the pivoted route)
  lu32_refine = inf == 0 && r >= 1e-2 && r < 0.5;
  if (verbose)
    std::printf("mg: coarse FP32 unpivoted LU n=%lld info=%d, check |A x - 1| / |1| = %.2e%s\n", (long long)n, inf, r,
                lu32_refine ? ", applied with one refinement step" : "");
  if (inf == 0 && r < 0.5) return GLS_OK;
  lu32_npvt = lu32_refine = false;
  HIP_TRY(gls::vec_to_f32(probe.p, probe32.p, n * n, s));  // the pinned matrix again
  const int rc = invert(s, probe32.p, true, &inf);
  if (rc < 0) return rc;
  if (verbose) std::printf("mg: coarse FP32 pivoted LU + inverse n=%lld info=%d\n", (long long)n, inf);
  if (inf != 0) {
    ok = lu32 = false;
    return set_err(GLS_EINVAL, "coarse FP32 LU: zero pivot %d", inf);
  }
  return GLS_OK;
}

int CoarseSolve::solve(hipStream_t s, const double *b, double *x, const int32_t *perm) {
  const rocblas_int N = (rocblas_int)n;
  if (band_store) {  // the band-storage factor, in the CSR's Cuthill-McKee order
    HIP_TRY(gls::vec_permute(tmp.p, b, perm, n, 0, s));
    GLS_TRY(blu.solve(s, tmp.p, tmp.p, lu32_refine));
    HIP_TRY(gls::vec_permute(x, tmp.p, perm, n, 1, s));
    HIP_TRY(hipMemsetAsync(x + pin_dof, 0, sizeof(double), s));  // pinned: no correction
    return GLS_OK;
  }
  if (lu32) {  // the FP32 factor / inverse, in the matrix's order (banded: the CSR's Cuthill-McKee order)
    const double *bb = b;
    double *xx = x;
    if (banded) {
      HIP_TRY(gls::vec_permute(tmp.p, b, perm, n, 0, s));
      bb = xx = tmp.p;
    }
    if (lu32_npvt) {  // x = U^-1 L^-1 b
      const int bl = banded ? (int)band.bl : -1, bu = banded ? (int)band.bu : -1;
      HIP_TRY(gls::vec_to_f32(bb, x32.p, n, s));
      HIP_TRY(gls::dense_lu_solve_f32(probe32.p, (int)n, x32.p, s, bl, bu));
      if (lu32_refine) {  // r = b - A x (the pinned FP64 matrix), x += LU^-1 r
        const double one = 1.0, mone = -1.0;
        double *r = chk32.p, *x0 = chk32.p + n;
        HIP_TRY(gls::vec_from_f32(x32.p, x0, n, s));
        HIP_TRY(gls::vec_copy(r, bb, n, s));
        if (rocblas_set_stream(blas.get(), s) != kOk ||
            rocblas_dgemv(blas.get(), rocblas_operation_none, N, N, &mone, probe.p, N, x0, 1, &one, r, 1) != kOk)
          return set_err(GLS_EHIP, "rocblas_dgemv failed");
        HIP_TRY(gls::vec_to_f32(r, x32.p, n, s));
        HIP_TRY(gls::dense_lu_solve_f32(probe32.p, (int)n, x32.p, s, bl, bu));
        HIP_TRY(gls::vec_from_f32(x32.p, xx, n, s));
        HIP_TRY(gls::vec_axpy(xx, 1.0, x0, n, s));
      } else {
        HIP_TRY(gls::vec_from_f32(x32.p, xx, n, s));
      }
    } else {  // x = A^-1 b
      const float one = 1.0f, zero = 0.0f;
      HIP_TRY(gls::vec_to_f32(bb, b32.p, n, s));
      if (rocblas_set_stream(blas.get(), s) != kOk ||
          rocblas_sgemv(blas.get(), rocblas_operation_none, N, N, &one, probe32.p, N, b32.p, 1, &zero, x32.p, 1) != kOk)
        return set_err(GLS_EHIP, "rocblas_sgemv failed");
      HIP_TRY(gls::vec_from_f32(x32.p, xx, n, s));
    }
    if (banded) HIP_TRY(gls::vec_permute(x, tmp.p, perm, n, 1, s));
    HIP_TRY(hipMemsetAsync(x + pin_dof, 0, sizeof(double), s));  // pinned: no correction
    return GLS_OK;
  }
  if (lu) {  // the explicit FP64 inverse (its pinned row zeroed by factor)
    const double one = 1.0, zero = 0.0;
    if (rocblas_set_stream(blas.get(), s) != kOk ||
        rocblas_dgemv(blas.get(), rocblas_operation_none, N, N, &one, probe.p, N, b, 1, &zero, x, 1) != kOk)
      return set_err(GLS_EHIP, "rocblas_dgemv failed");
    return GLS_OK;
  }
  HIP_TRY(gls::mg_dense_apply(aug.p, (int)n, b, x, s));  // Gauss-Jordan
  return GLS_OK;
}

}  // namespace gls_impl
