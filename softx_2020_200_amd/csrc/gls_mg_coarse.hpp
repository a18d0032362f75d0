// gls_mg_coarse.hpp -- internal: the multigrid's coarsest-level direct solve (gls_mg_coarse.cpp). CoarseSolve owns
// the dense matrix, its factors, the scratch vectors, the rocBLAS handle and the side stream with its worker thread;
// it sees an n x n column-major array (and, for a banded matrix, its bandwidths and permutation), never a context:
// the multigrid (gls_mg.cpp) probes the level's Jacobian into matrix() and calls factor / finish / solve.
// Above kDirectMax unknowns (or when asked) the n x n arrays give way to band storage filled from the probed CSR
// (init_band / factor_band, gls_band_lu.hpp); finish and solve are the same calls.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <memory>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>

#include <rocblas/rocblas.h>

#include "gls_band_lu.hpp"
#include "gls_devbuf.hpp"

namespace gls_impl {

constexpr int64_t kDirectSmall = 8192, kDirectMax = 40000;  // coarsest-level dense LU: FP64 / FP32 ranges

struct CoarseSolve {
  using Clock = std::chrono::steady_clock;
  int64_t n = 0;    // the matrix's order (init)
  bool ok = false;  // this state's factorization stands: solve() applies it
  // n <= kDirectSmall: LU (rocSOLVER getrf + getri -> explicit inverse, applied by rocBLAS gemv) with the first
  // pressure DoF pinned (enclosed-flow gauge); GLS_MG_COARSE_SOLVER=gj: the one-workgroup Gauss-Jordan
  // (mg_dense_invert) instead
  bool lu = false;
  // large coarsest levels (kDirectSmall < n <= kDirectMax, e.g. a Q1-Q1 p-level of a 4.7 k-cell base mesh):
  // the pinned FP64 matrix rounded to FP32, pivoted sgetrf + sgetri, applied by sgemv (a preconditioner's
  // coarse solve: FP32 rounding of A^-1 is far below the V-cycle's own error; half the bytes and the FP32
  // matrix-core rate for the O(n^3) setup)
  bool lu32 = false;
  bool lu32_npvt = false;  // the FP32 factor is unpivoted (applied by dense_lu_solve_f32), else an explicit inverse
  bool lu32_refine = false;  // ... applied with one step of iterative refinement against the FP64 matrix
  // banded coarse matrix: the probed CSR's Cuthill-McKee order kept (the dense array holds A in that order), its
  // lower / upper bandwidths and the pinned DoF's row, set by the prober once (bl < 0: not yet); the factorization
  // works by column blocks as wide as the band (no fill outside it without pivoting) and the solves skip the blocks
  // outside it. configs[4]'s 25 k-DoF Q1-Q1 p-level: ~1.9 k
  struct Band {
    int64_t bl = -1, bu = -1, pin = -1;
  } band;
  bool banded = false;  // this state's matrix is in that order (factor)
  DevBuf<int32_t> ident;  // the prober's identity permutation (csr_to_dense in the CSR's own order)
  DevBuf<int32_t> pinv;   // ... and csr_to_dense's inverse permutation
  DevBuf<double> tmp;     // the coarse right-hand side / correction in the band order
  DevBuf<float> probe32, b32, x32;
  DevBuf<double> chk32;    // the FP32 factor's check: A x - b for b = 1 (FP64)
  int64_t npvt_ipiv_n = -1;  // ipiv holds the identity permutation of this size (unpivoted LU)
  struct BlasDestroy {
    void operator()(rocblas_handle h) const { rocblas_destroy_handle(h); }
  };
  std::unique_ptr<std::remove_pointer_t<rocblas_handle>, BlasDestroy> blas;  // owning rocBLAS handle
  DevBuf<int> ipiv, info;
  DevBuf<double> probe, aug, unit;
  DevBuf<double> probe_bak;  // the probed coarse matrix kept for the pivoted retry of an unpivoted LU
  DevBuf<double> chk;        // inverse_check's y = A^-1 e and z = A y
  DevBuf<int> status;
  bool pending = false;  // side-stream factorization in flight, not yet checked (finish)
  int64_t pin_dof = 0;   // the pinned unknown (first pressure DoF) and its row in the matrix's order
  int64_t pin_row() const { return banded ? band.pin : pin_dof; }
  DevBuf<double> rel;    // |A x - 1| of the FP32 check (device pointer mode)
  // the band route (init_band): the FP32 matrix in block-tridiagonal storage filled from the probing ILU's CSR
  // (gls_band_lu.hpp), for levels whose n x n arrays do not fit -- probe / probe32 stay empty. Factored on the side
  // stream by the worker like the dense FP32 route, checked and refined against the FP64 CSR; no pivoted fallback
  bool band_store = false;
  BandLU blu;
  Clock::time_point t_getrf;  // when invert()'s last getrf had returned its info (verbose timings)
  // the FP32 unpivoted factorization and its check run on a stream of their own, overlapping the finer levels'
  // ILU setup and first smoothing on the context stream; the first coarse solve waits for them (finish).
  // rocSOLVER's getrf returns to the host only when the factorization is done (82-89 ms of host time at
  // n = 25000, box r06v), so the calls are made from a worker thread: the host thread queues the finer levels'
  // setup meanwhile. Side is the LAST member and the destructor and the move assignment reset it first: the worker
  // is joined and its stream drained before any buffer it reads or writes (rel included) is released.
  struct Side {
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::thread worker;
    int rc = 0;  // the worker's result: 0, or the failing call's number
    Side() = default;
    Side(const Side &) = delete;
    Side &operator=(const Side &) = delete;
    Side(Side &&o) noexcept : s(o.s), e0(o.e0), e1(o.e1), worker(std::move(o.worker)), rc(o.rc) {
      o.s = nullptr, o.e0 = o.e1 = nullptr;
    }
    void join() {
      if (worker.joinable()) worker.join();
    }
    hipError_t ensure() {
      if (s) return hipSuccess;
      hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&e0, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&e1, hipEventDisableTiming);
      return e;
    }
    void reset() {
      join();
      if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
      }
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      s = nullptr, e0 = e1 = nullptr;
    }
    ~Side() { reset(); }
  } side;

  CoarseSolve() = default;
  CoarseSolve(CoarseSolve &&) noexcept = default;
  // the worker holds a pointer to the struct it was started from, so both sides' workers end before anything moves
  CoarseSolve &operator=(CoarseSolve &&o) noexcept {
    if (this != &o) {
      side.reset();
      o.side.reset();
      this->~CoarseSolve();
      new (this) CoarseSolve(std::move(o));
    }
    return *this;
  }
  ~CoarseSolve() { side.reset(); }

  // the one allocation routine (both attach paths): the FP64 matrix and pivots, the FP32 copies above kDirectSmall,
  // the Gauss-Jordan buffer whenever GLS_MG_COARSE_SOLVER is set, the rocBLAS handle
  int init(int64_t n);
  // the band route's allocations instead: the panels for the bandwidths in band (set by the prober), no dense array
  int init_band(int64_t n, int64_t block);
  // ... and its factorization: the panels filled from the CSR (device, in the band's order, unchanged until the next
  // preparation) on s, the block LU and its check handed to the worker
  int factor_band(hipStream_t s, const int64_t *rowp, const int32_t *col, const double *val, int64_t pin, Clock::time_point t0);
  double *matrix() { return probe.p; }  // the prober writes the dense FP64 matrix here (column-major n x n)
  // factor the probed matrix on s with the DoF pin pinned; banded_: the matrix is in the band's order. The route by n
  // and GLS_MG_COARSE_SOLVER (gj | lu | lu_npvt): up to kDirectSmall in place and checked, above rounded to FP32 and
  // handed to the worker (nothing waits on the host). t0: the preparation's start, for the GLS_MG_VERBOSE timings
  int factor(hipStream_t s, int64_t pin, bool banded_, Clock::time_point t0);
  // before the first solve of a state: the side stream's factorization checked, the pivoted FP32 route on s where
  // pivot growth broke it. No-op unless one is pending; on an error ok is cleared (the caller prepares again)
  int finish(hipStream_t s);
  // x = A^-1 b by the route factor() took, the pinned unknown zero; perm: DoF -> row of a banded matrix
  int solve(hipStream_t s, const double *b, double *x, const int32_t *perm);

 private:
  template <class T>
  int invert(hipStream_t s, T *A, bool pivot, int *inf);
  int inverse_check(hipStream_t s, bool *good);
  int factor_f64(hipStream_t s, const char *route, Clock::time_point t0, Clock::time_point t1);
  int start_f32(hipStream_t s);
  int finish_band();
};

}  // namespace gls_impl
