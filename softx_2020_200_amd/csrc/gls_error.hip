// gls_error.hip -- the L2 error of a solution vector against an analytical solution (the reference's
// calculate_L2_error, restated by the application's host l2_error()): QGauss(k+2) on every cell, the exact solution
// from the expression's bytecode at the mapped points and the time t, the pressures compared mean-free.
//   pass 1: int p_h, int p, volume          pass 2: int |u_h - u|^2, int ((p_h - mean p_h) - (p - mean p))^2
// Pass 2 reads pass 1's three sums, as the host does: two launches, not the one-pass identity int d^2 - (int d)^2 / V,
// which cancels (the discrete pressure is fixed only up to a constant).
//
// Work decomposition: one lane per quadrature point, the cells packed into the block as in gls_output.hip: a block
// takes cpb consecutive cells and lane t is point t % nq of cell t / nq; nq = (k+2)^dim is 9, 16, 27 or 64, so a 3D
// Q2 cell is exactly one wave. The velocity and the pressure are evaluated by value only, sum-factorized through
// LDS with the block sharing each sweep (gls_lattice_eval.hpp); no gradients. Then the lane runs the interpreter
// (gls_expr_device.hpp) on its own x and the scalar t -- no variable array is materialised -- and forms its
// contribution.
//
// Geometry: Gauss points are not the context's QGauss(k+1) points, so the geometry is the plan's. Box cells:
// x = x0 + h xq, JxW = prod h_d w_d (the host's expressions). Mapped cells: x and J = d x / d xi from the
// MappingQ support points as dim more fields of the same sweeps, JxW = det J w; J^-1 is not needed.
//
// Reduction: no atomics. Each block folds its lanes' three values in LDS (a halving tree: a fixed order) into
// partial[block][3]; one finishing block gives each lane the partials block = lane, lane + 256, ... in ascending
// order and folds the lanes with the same tree. Two calls on the same input are bitwise equal, and a context's
// layout (brick, per cell, mapped, hanging lines) enters only through cell_vnodes / cell_pnodes.
// Instantiated for dim 2, 3 x (k, kp) in {(1,1), (2,1), (2,2)} x box / mapped x pass; the mapping degree is a
// run-time value (<= 3).
#include "gls_expr_device.hpp"
#include "gls_lattice_eval.hpp"
#include "gls_launch.hpp"

namespace gls {

namespace {

constexpr int kErrMaxBlock = 256;             // lanes per block at most
constexpr int kErrLdsDoubles = 64 * 1024 / 8;  // LDS budget of one block
constexpr int kErrSums = 3;

struct ErrorArgs {
  const int32_t *cell_vnodes, *cell_pnodes;
  const double *sol;
  int64_t pbase;          // the pressure of node n is sol[pbase + n]
  const double *x0h;      // box cells: [n_cells][2 dim] = x0 | h
  const double *support;  // mapped cells: [n_cells][nm^dim][dim]
  const double *tab;      // Vv [nq1][k+1] | Vp [nq1][kp+1] | xq [nq1] | wq [nq1] | Vm [nq1][nm] | Dm
  int64_t n_cells;
  int nm, cpb;
  expr::DeviceProgram exact;
  double time;
  const double *means;    // pass 2: int p_h, int p, volume (pass 1's result)
  double *partial;        // [blocks][3]
};

// fold the block's values into lane 0 (the block has 64, 128, 192 or 256 lanes); red: [3][blockDim.x]
__device__ __forceinline__ void block_fold(double (&v)[kErrSums], double *red) {
  const int tid = threadIdx.x, nthr = blockDim.x;
#pragma unroll
  for (int i = 0; i < kErrSums; ++i) red[i * nthr + tid] = v[i];
  __syncthreads();
  for (int st = kErrMaxBlock / 2; st > 0; st >>= 1) {
    if (tid < st && tid + st < nthr) {
#pragma unroll
      for (int i = 0; i < kErrSums; ++i) red[i * nthr + tid] += red[i * nthr + tid + st];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kErrSums; ++i) v[i] = red[i * nthr];
}

template <int DIM, int K, int KP, bool MAPPED, int PASS>
__global__ void __launch_bounds__(kErrMaxBlock) k_l2_error(const ErrorArgs A) {
  constexpr int K1 = K + 1, KP1 = KP + 1, NV = opow(K1, DIM), NP = opow(KP1, DIM);
  constexpr int NQ1 = K + 2, NQ = opow(NQ1, DIM);
  extern __shared__ double lds[];
  const int nm = A.nm, nsup = opow(nm, DIM);
  const int tid = threadIdx.x, nthr = blockDim.x;
  // LDS: tables | reduction [3][nthr] | operand stack [max_stack][nthr] | per cell: velocity fields, pressure, support
  const int ntab = NQ1 * (K1 + KP1 + 2 + (MAPPED ? 2 * nm : 0));
  double *tVv = lds, *tVp = tVv + NQ1 * K1, *tX = tVp + NQ1 * KP1, *tW = tX + NQ1, *tVm = tW + NQ1, *tDm = tVm + NQ1 * nm;
  double *red = lds + ntab, *stack = red + kErrSums * nthr, *cells = stack + A.exact.max_stack * nthr;
  const int fv = field_doubles(DIM, K1, NQ1, false), fp = field_doubles(DIM, KP1, NQ1, false),
            fm = MAPPED ? field_doubles(DIM, nm, NQ1, true) : 0;
  const int off_p = DIM * fv, off_m = off_p + fp, cs = off_m + DIM * fm;
  const int64_t cell0 = (int64_t)blockIdx.x * A.cpb;
  const int ncl = (int)(A.n_cells - cell0 < A.cpb ? A.n_cells - cell0 : A.cpb);

  for (int i = tid; i < ntab; i += nthr) lds[i] = A.tab[i];
  // gather: velocity [cl][a][c] (the components of a node are adjacent in sol; pass 1 needs the pressure only)
  if constexpr (PASS == 2) {
    for (int i = tid; i < ncl * NV * DIM; i += nthr) {
      const int cl = i / (NV * DIM), r = i - cl * (NV * DIM), a = r / DIM, c = r - a * DIM;
      const int64_t node = A.cell_vnodes[(cell0 + cl) * NV + a];
      cells[cl * cs + c * fv + a] = A.sol[node * DIM + c];
    }
  }
  for (int i = tid; i < ncl * NP; i += nthr) {
    const int cl = i / NP, a = i - cl * NP;
    cells[cl * cs + off_p + a] = A.sol[A.pbase + A.cell_pnodes[(cell0 + cl) * NP + a]];
  }
  if constexpr (MAPPED) {
    for (int i = tid; i < ncl * nsup * DIM; i += nthr) {
      const int cl = i / (nsup * DIM), r = i - cl * (nsup * DIM), b = r / DIM, c = r - b * DIM;
      cells[cl * cs + off_m + c * fm + b] = A.support[(cell0 + cl) * nsup * DIM + r];
    }
  }
  __syncthreads();
  if constexpr (PASS == 2) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_a<DIM, false>(cells + c * fv, cs, ncl, K1, NQ1, tVv, nullptr);
  }
  sweep_a<DIM, false>(cells + off_p, cs, ncl, KP1, NQ1, tVp, nullptr);
  if constexpr (MAPPED) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_a<DIM, true>(cells + off_m + c * fm, cs, ncl, nm, NQ1, tVm, tDm);
  }
  __syncthreads();
  if constexpr (DIM == 3) {
    if constexpr (PASS == 2) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) sweep_b<false>(cells + c * fv, cs, ncl, K1, NQ1, tVv, nullptr);
    }
    sweep_b<false>(cells + off_p, cs, ncl, KP1, NQ1, tVp, nullptr);
    if constexpr (MAPPED) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) sweep_b<true>(cells + off_m + c * fm, cs, ncl, nm, NQ1, tVm, tDm);
    }
    __syncthreads();
  }

  double val[kErrSums] = {0.0, 0.0, 0.0};
  if (tid < ncl * NQ) {
    const int cl = tid / NQ, q = tid - cl * NQ;
    const int tt[3] = {q % NQ1, (q / NQ1) % NQ1, DIM == 3 ? q / (NQ1 * NQ1) : 0};
    const double *cf = cells + cl * cs;
    double u[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0}, ph, JxW, dummy[3];
    if constexpr (PASS == 2) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) finish<DIM, false>(cf + c * fv, K1, NQ1, tt, tVv, nullptr, u[c], dummy);
    }
    finish<DIM, false>(cf + off_p, KP1, NQ1, tt, tVp, nullptr, ph, dummy);
    if constexpr (MAPPED) {
      double J[3][3];  // J[i][a] = d x_i / d xi_a
#pragma unroll
      for (int i = 0; i < DIM; ++i) finish<DIM, true>(cf + off_m + i * fm, nm, NQ1, tt, tVm, tDm, x[i], J[i]);
      double det;
      if constexpr (DIM == 2)
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      else
        det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
              J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      JxW = det * tW[tt[0]] * tW[tt[1]] * (DIM == 3 ? tW[tt[2]] : 1.0);
    } else {
#pragma clang fp contract(off)  // the host's x = x0 + h xq: two rounded operations
      const double *xh = A.x0h + (cell0 + cl) * 2 * DIM;
      JxW = 1.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const double h = xh[DIM + d];
        x[d] = xh[d] + h * tX[tt[d]];
        JxW *= h * tW[tt[d]];
      }
    }
    const expr::DeviceProgram &E = A.exact;
    const double t = A.time;
    auto var = [&](int i) { return i == 0 ? x[0] : i == 1 ? x[1] : (DIM == 3 && i == 2) ? x[2] : t; };
    double *st = stack + tid;
    // an expression with only dim components has exact pressure 0
    const double pe = E.n_comps > DIM ? expr::run(E.code, E.off[DIM], E.off[DIM + 1], st, nthr, var) : 0.0;
    if constexpr (PASS == 1) {
      val[0] = ph * JxW;
      val[1] = pe * JxW;
      val[2] = JxW;
    } else {
      const double pint = A.means[0], peint = A.means[1], vol = A.means[2];
      double eu = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const double ex = expr::run(E.code, E.off[d], E.off[d + 1], st, nthr, var);
        eu += (u[d] - ex) * (u[d] - ex) * JxW;
      }
      const double dp = (ph - pint / vol) - (pe - peint / vol);
      val[0] = eu;
      val[1] = dp * dp * JxW;
    }
  }
  block_fold(val, red);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < kErrSums; ++i) A.partial[(int64_t)blockIdx.x * kErrSums + i] = val[i];
  }
}

// out[3] = the block partials folded: lane l takes blocks l, l + 256, ... in ascending order. volume >= 0 replaces
// out[2] (general meshes: the sum of the Q1 cell measures, GridTools::volume)
__global__ void __launch_bounds__(kErrMaxBlock)
    k_l2_error_finish(const double *__restrict__ partial, int64_t n_blocks, double volume, double *__restrict__ out) {
  __shared__ double red[kErrSums * kErrMaxBlock];
  double val[kErrSums] = {0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < n_blocks; b += kErrMaxBlock) {
#pragma unroll
    for (int i = 0; i < kErrSums; ++i) val[i] += partial[b * kErrSums + i];
  }
  block_fold(val, red);
  if (threadIdx.x == 0) {
    out[0] = val[0];
    out[1] = val[1];
    out[2] = volume >= 0.0 ? volume : val[2];
  }
}

// cells per block, lanes per block and LDS bytes; false: no launch shape exists
bool error_shape(int dim, int k, int kp, int nm, int max_stack, int &cpb, int &threads, size_t &lds_bytes) {
  const int nq1 = k + 2, nq = opow(nq1, dim);
  const int per_cell = dim * field_doubles(dim, k + 1, nq1, false) + field_doubles(dim, kp + 1, nq1, false) +
                       (nm ? dim * field_doubles(dim, nm, nq1, true) : 0);
  const int ntab = nq1 * ((k + 1) + (kp + 1) + 2 + 2 * nm);
  for (cpb = kErrMaxBlock / nq; cpb >= 1; --cpb) {
    threads = (cpb * nq + 63) / 64 * 64;
    const int total = ntab + (kErrSums + max_stack) * threads + cpb * per_cell;
    if (total <= kErrLdsDoubles) {
      lds_bytes = sizeof(double) * (size_t)total;
      return true;
    }
  }
  return false;
}

}  // namespace

bool l2_error_supported(int dim, int k, int kp, int map_degree, int max_stack) {
  int cpb, threads;
  size_t lds;
  return (dim == 2 || dim == 3) && ((k == 1 && kp == 1) || (k == 2 && kp == 1) || (k == 2 && kp == 2)) &&
         map_degree >= 0 && map_degree <= 3 && max_stack >= 1 && max_stack <= expr::kDeviceMaxStack &&
         error_shape(dim, k, kp, map_degree ? map_degree + 1 : 0, max_stack, cpb, threads, lds);
}

int64_t l2_error_blocks(int dim, int k, int kp, int map_degree, int max_stack, int64_t n_cells) {
  int cpb = 1, threads;
  size_t lds;
  if (!error_shape(dim, k, kp, map_degree ? map_degree + 1 : 0, max_stack, cpb, threads, lds)) return 0;
  return (n_cells + cpb - 1) / cpb;
}

hipError_t launch_l2_error(int dim, int k, int kp, int map_degree, const int32_t *cell_vnodes, const int32_t *cell_pnodes,
                           const double *sol, int64_t pbase, const double *x0h, const double *support, const double *tab,
                           int64_t n_cells, const expr::DeviceProgram &exact, double time, double volume, double *partial,
                           double *out, hipStream_t s) {
  if (!l2_error_supported(dim, k, kp, map_degree, exact.max_stack)) return hipErrorNotSupported;
  if (n_cells <= 0 || (map_degree ? !support : !x0h) || exact.n_comps < dim || exact.n_vars != dim + 1)
    return hipErrorInvalidValue;
  ErrorArgs A;
  A.cell_vnodes = cell_vnodes;
  A.cell_pnodes = cell_pnodes;
  A.sol = sol;
  A.pbase = pbase;
  A.x0h = x0h;
  A.support = support;
  A.tab = tab;
  A.n_cells = n_cells;
  A.nm = map_degree ? map_degree + 1 : 0;
  A.exact = exact;
  A.time = time;
  A.means = out;
  A.partial = partial;
  int threads;
  size_t lds;
  error_shape(dim, k, kp, A.nm, exact.max_stack, A.cpb, threads, lds);
  const int64_t nb = (n_cells + A.cpb - 1) / A.cpb;
  const dim3 g((unsigned)nb), b((unsigned)threads);
  // pass 1 -> out[0..2], pass 2 (reads out[0..2]) -> out[3..5]
#define GLS_ERR_CASE(D, KK, KKP)                                                                     \
  if (dim == D && k == KK && kp == KKP) {                                                            \
    if (map_degree)                                                                                  \
      hipLaunchKernelGGL((k_l2_error<D, KK, KKP, true, 1>), g, b, lds, s, A);                        \
    else                                                                                             \
      hipLaunchKernelGGL((k_l2_error<D, KK, KKP, false, 1>), g, b, lds, s, A);                       \
    hipError_t e = hipGetLastError();                                                                \
    if (e != hipSuccess) return e;                                                                   \
    hipLaunchKernelGGL(k_l2_error_finish, dim3(1), dim3(kErrMaxBlock), 0, s, partial, nb, volume, out); \
    if (map_degree)                                                                                  \
      hipLaunchKernelGGL((k_l2_error<D, KK, KKP, true, 2>), g, b, lds, s, A);                        \
    else                                                                                             \
      hipLaunchKernelGGL((k_l2_error<D, KK, KKP, false, 2>), g, b, lds, s, A);                       \
    e = hipGetLastError();                                                                           \
    if (e != hipSuccess) return e;                                                                   \
    hipLaunchKernelGGL(k_l2_error_finish, dim3(1), dim3(kErrMaxBlock), 0, s, partial, nb, -1.0, out + kErrSums); \
  }
  GLS_ERR_CASE(2, 1, 1)
  GLS_ERR_CASE(2, 2, 1)
  GLS_ERR_CASE(2, 2, 2)
  GLS_ERR_CASE(3, 1, 1)
  GLS_ERR_CASE(3, 2, 1)
  GLS_ERR_CASE(3, 2, 2)
#undef GLS_ERR_CASE
  return hipGetLastError();
}

}  // namespace gls
