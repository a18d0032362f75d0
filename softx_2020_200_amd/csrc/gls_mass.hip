// gls_mass.hip -- the consistent mass matrix of the velocity-pressure space, matrix-free (the reference's
// assemble_L2_projection, gls_navier_stokes.cc:830-914, never assembled): QGauss(k+1) on every cell, the dim
// velocity components and the pressure as dim + 1 scalar fields.
//   apply:     y_e = M_e x_e                       gather, forward sweeps, * JxW, transposed sweeps
//   rhs:       b_e = int phi f(x, t) JxW           f from the expression's bytecode at the lane's own x and t
//   diagonal:  d_a = sum_q phi_a(q)^2 JxW          the transposed sweeps with the squared 1D tables on JxW alone
//
// Work decomposition: gls_error.hip's. One lane per quadrature point, a block takes cpb consecutive cells and lane t
// is point t % nq of cell t / nq; nq = (k+1)^dim is 4, 9, 8 or 27. Tables and per-cell fields sit in LDS and the
// sweeps (gls_lattice_eval.hpp) are shared by the whole block. A field of a cell owns nodal | A | B | q: the forward
// sweeps go nodal -> A -> B -> the lane's value, the lane stores value * JxW into q, the transposed sweeps go
// q -> B -> A -> nodal. (dim+1) * 2 * dim * (k+1) FMAs per point, not the 2 (k+1)^dim of a dense loop.
//
// Geometry: the plan's, as in gls_error.hip. Box cells: x = x0 + h xq, JxW = prod h_d w_d. Mapped cells: x and
// J = d x / d xi from the MappingQ support points as dim more swept fields, JxW = det J w.
//
// Output: element vectors [cell][NV * dim + NP] (velocity slot a, component c at a * dim + c; pressure slot a at
// NV * dim + a), the per-cell kernels' layout: gather_element_vectors sums a node's slots in ascending cell order.
// No atomics; two launches on the same input are bitwise equal, and a context's layout (brick, per cell, mapped)
// enters only through cell_vnodes / cell_pnodes.
// Instantiated for dim 2, 3 x (k, kp) in {(1,1), (2,1), (2,2)} x box / mapped x the three modes; the mapping degree
// is a run-time value (<= 3).
#include "gls_expr_device.hpp"
#include "gls_lattice_eval.hpp"
#include "gls_launch.hpp"

namespace gls {

namespace {

constexpr int kMassMaxBlock = 256;              // lanes per block at most
constexpr int kMassLdsDoubles = 64 * 1024 / 8;  // LDS budget of one block

struct MassArgs {
  const int32_t *cell_vnodes, *cell_pnodes;
  const double *x;        // apply: the vector; the pressure of node n is x[pbase + n]
  int64_t pbase;
  const double *x0h;      // box cells: [n_cells][2 dim] = x0 | h
  const double *support;  // mapped cells: [n_cells][nm^dim][dim]
  const double *tab;      // Vv [nq1][k+1] | Vp [nq1][kp+1] | xq [nq1] | wq [nq1] | Vv^2 | Vp^2 | Vm [nq1][nm] | Dm
  int64_t n_cells;
  int nm, cpb, max_stack;
  expr::DeviceProgram f;  // rhs
  double time;
  double *ev;             // [n_cells][NV dim + NP]
};

// LDS doubles of one value field of one cell with its point array: nodal | A | B | q
__host__ __device__ inline int mass_field_doubles(int dim, int n, int np1) {
  return field_doubles(dim, n, np1, false) + opow(np1, dim);
}

template <int DIM, int K, int KP, bool MAPPED, int MODE>
__global__ void __launch_bounds__(kMassMaxBlock) k_mass(const MassArgs A) {
  constexpr int K1 = K + 1, KP1 = KP + 1, NV = opow(K1, DIM), NP = opow(KP1, DIM), EL = NV * DIM + NP;
  constexpr int NQ1 = K + 1, NQ = opow(NQ1, DIM);
  extern __shared__ double lds[];
  const int nm = A.nm, nsup = opow(nm, DIM);
  const int tid = threadIdx.x, nthr = blockDim.x;
  // LDS: tables | operand stack [max_stack][nthr] (rhs) | per cell: velocity fields, pressure, support
  const int ntab = NQ1 * (2 * K1 + 2 * KP1 + 2 + (MAPPED ? 2 * nm : 0));
  double *tVv = lds, *tVp = tVv + NQ1 * K1, *tX = tVp + NQ1 * KP1, *tW = tX + NQ1, *tVv2 = tW + NQ1,
         *tVp2 = tVv2 + NQ1 * K1, *tVm = tVp2 + NQ1 * KP1, *tDm = tVm + NQ1 * nm;
  double *stack = lds + ntab, *cells = stack + (MODE == kMassRhs ? A.max_stack * nthr : 0);
  const int fv = mass_field_doubles(DIM, K1, NQ1), fp = mass_field_doubles(DIM, KP1, NQ1),
            fm = MAPPED ? field_doubles(DIM, nm, NQ1, true) : 0;
  const int qv = fv - NQ, qp = fp - NQ;  // the point arrays inside the regions
  const int off_p = DIM * fv, off_m = off_p + fp, cs = off_m + DIM * fm;
  const int64_t cell0 = (int64_t)blockIdx.x * A.cpb;
  const int ncl = (int)(A.n_cells - cell0 < A.cpb ? A.n_cells - cell0 : A.cpb);

  for (int i = tid; i < ntab; i += nthr) lds[i] = A.tab[i];
  if constexpr (MODE == kMassApply) {  // gather: velocity [cl][a][c] (the components of a node are adjacent in x)
    for (int i = tid; i < ncl * NV * DIM; i += nthr) {
      const int cl = i / (NV * DIM), r = i - cl * (NV * DIM), a = r / DIM, c = r - a * DIM;
      const int64_t node = A.cell_vnodes[(cell0 + cl) * NV + a];
      cells[cl * cs + c * fv + a] = A.x[node * DIM + c];
    }
    for (int i = tid; i < ncl * NP; i += nthr) {
      const int cl = i / NP, a = i - cl * NP;
      cells[cl * cs + off_p + a] = A.x[A.pbase + A.cell_pnodes[(cell0 + cl) * NP + a]];
    }
  }
  if constexpr (MAPPED) {
    for (int i = tid; i < ncl * nsup * DIM; i += nthr) {
      const int cl = i / (nsup * DIM), r = i - cl * (nsup * DIM), b = r / DIM, c = r - b * DIM;
      cells[cl * cs + off_m + c * fm + b] = A.support[(cell0 + cl) * nsup * DIM + r];
    }
  }
  __syncthreads();
  if constexpr (MODE == kMassApply) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_a<DIM, false>(cells + c * fv, cs, ncl, K1, NQ1, tVv, nullptr);
    sweep_a<DIM, false>(cells + off_p, cs, ncl, KP1, NQ1, tVp, nullptr);
  }
  if constexpr (MAPPED) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_a<DIM, true>(cells + off_m + c * fm, cs, ncl, nm, NQ1, tVm, tDm);
  }
  if constexpr (MODE == kMassApply || MAPPED) __syncthreads();
  if constexpr (DIM == 3) {
    if constexpr (MODE == kMassApply) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) sweep_b<false>(cells + c * fv, cs, ncl, K1, NQ1, tVv, nullptr);
      sweep_b<false>(cells + off_p, cs, ncl, KP1, NQ1, tVp, nullptr);
    }
    if constexpr (MAPPED) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) sweep_b<true>(cells + off_m + c * fm, cs, ncl, nm, NQ1, tVm, tDm);
    }
    if constexpr (MODE == kMassApply || MAPPED) __syncthreads();
  }

  // the lane's point: the dim + 1 values times JxW into the point arrays (regions of their own: no barrier before)
  if (tid < ncl * NQ) {
    const int cl = tid / NQ, q = tid - cl * NQ;
    const int tt[3] = {q % NQ1, (q / NQ1) % NQ1, DIM == 3 ? q / (NQ1 * NQ1) : 0};
    double *cf = cells + cl * cs;
    double x[3] = {0.0, 0.0, 0.0}, JxW, dummy[3];
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
    if constexpr (MODE == kMassApply) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        double u;
        finish<DIM, false>(cf + c * fv, K1, NQ1, tt, tVv, nullptr, u, dummy);
        cf[c * fv + qv + q] = u * JxW;
      }
      double p;
      finish<DIM, false>(cf + off_p, KP1, NQ1, tt, tVp, nullptr, p, dummy);
      cf[off_p + qp + q] = p * JxW;
    } else if constexpr (MODE == kMassRhs) {
      const expr::DeviceProgram &E = A.f;
      const double t = A.time;
      auto var = [&](int i) { return i == 0 ? x[0] : i == 1 ? x[1] : (DIM == 3 && i == 2) ? x[2] : t; };
      double *st = stack + tid;
#pragma unroll
      for (int c = 0; c < DIM; ++c) cf[c * fv + qv + q] = expr::run(E.code, E.off[c], E.off[c + 1], st, nthr, var) * JxW;
      cf[off_p + qp + q] = expr::run(E.code, E.off[DIM], E.off[DIM + 1], st, nthr, var) * JxW;
    } else {  // the diagonal: one velocity field serves the dim components
      cf[qv + q] = JxW;
      cf[off_p + qp + q] = JxW;
    }
  }
  __syncthreads();
  constexpr int NVF = MODE == kMassDiag ? 1 : DIM;  // velocity fields swept back
  const double *bV = MODE == kMassDiag ? tVv2 : tVv, *bP = MODE == kMassDiag ? tVp2 : tVp;
#pragma unroll
  for (int c = 0; c < NVF; ++c) sweep_t_last<DIM>(cells + c * fv, cells + c * fv + qv, cs, ncl, K1, NQ1, bV);
  sweep_t_last<DIM>(cells + off_p, cells + off_p + qp, cs, ncl, KP1, NQ1, bP);
  __syncthreads();
  if constexpr (DIM == 3) {
#pragma unroll
    for (int c = 0; c < NVF; ++c) sweep_t_b(cells + c * fv, cs, ncl, K1, NQ1, bV);
    sweep_t_b(cells + off_p, cs, ncl, KP1, NQ1, bP);
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < NVF; ++c) sweep_t_a<DIM>(cells + c * fv, cs, ncl, K1, NQ1, bV);
  sweep_t_a<DIM>(cells + off_p, cs, ncl, KP1, NQ1, bP);
  __syncthreads();
  // the element vectors: consecutive lanes store consecutive doubles
  double *ev = A.ev + cell0 * EL;
  for (int i = tid; i < ncl * EL; i += nthr) {
    const int cl = i / EL, r = i - cl * EL;
    double v;
    if (r < NV * DIM) {
      const int a = r / DIM, c = r - a * DIM;
      v = cells[cl * cs + (MODE == kMassDiag ? 0 : c) * fv + a];
    } else {
      v = cells[cl * cs + off_p + r - NV * DIM];
    }
    ev[i] = v;
  }
}

// cells per block, lanes per block and LDS bytes; false: no launch shape exists
bool mass_shape(int dim, int k, int kp, int nm, int max_stack, int &cpb, int &threads, size_t &lds_bytes) {
  const int nq1 = k + 1, nq = opow(nq1, dim);
  const int per_cell = dim * mass_field_doubles(dim, k + 1, nq1) + mass_field_doubles(dim, kp + 1, nq1) +
                       (nm ? dim * field_doubles(dim, nm, nq1, true) : 0);
  const int ntab = nq1 * (2 * (k + 1) + 2 * (kp + 1) + 2 + 2 * nm);
  for (cpb = kMassMaxBlock / nq; cpb >= 1; --cpb) {
    threads = (cpb * nq + 63) / 64 * 64;
    const int total = ntab + max_stack * threads + cpb * per_cell;
    if (total <= kMassLdsDoubles) {
      lds_bytes = sizeof(double) * (size_t)total;
      return true;
    }
  }
  return false;
}

}  // namespace

bool mass_supported(int dim, int k, int kp, int map_degree, int max_stack) {
  int cpb, threads;
  size_t lds;
  return (dim == 2 || dim == 3) && ((k == 1 && kp == 1) || (k == 2 && kp == 1) || (k == 2 && kp == 2)) &&
         map_degree >= 0 && map_degree <= 3 && max_stack >= 0 && max_stack <= expr::kDeviceMaxStack &&
         mass_shape(dim, k, kp, map_degree ? map_degree + 1 : 0, max_stack, cpb, threads, lds);
}

hipError_t launch_mass(int mode, int dim, int k, int kp, int map_degree, const int32_t *cell_vnodes,
                       const int32_t *cell_pnodes, const double *x, int64_t pbase, const double *x0h,
                       const double *support, const double *tab, int64_t n_cells, const expr::DeviceProgram *f,
                       double time, double *ev, hipStream_t s) {
  const int max_stack = mode == kMassRhs && f ? f->max_stack : 0;
  if (!mass_supported(dim, k, kp, map_degree, max_stack)) return hipErrorNotSupported;
  if (n_cells <= 0 || (map_degree ? !support : !x0h) || !tab || !ev || !cell_vnodes || !cell_pnodes ||
      (mode != kMassApply && mode != kMassRhs && mode != kMassDiag) || (mode == kMassApply && !x) ||
      (mode == kMassRhs && (!f || f->n_comps != dim + 1 || f->n_vars != dim + 1 || f->max_stack < 1)))
    return hipErrorInvalidValue;
  MassArgs A;
  A.cell_vnodes = cell_vnodes;
  A.cell_pnodes = cell_pnodes;
  A.x = x;
  A.pbase = pbase;
  A.x0h = x0h;
  A.support = support;
  A.tab = tab;
  A.n_cells = n_cells;
  A.nm = map_degree ? map_degree + 1 : 0;
  A.max_stack = max_stack;
  if (mode == kMassRhs) A.f = *f;
  A.time = time;
  A.ev = ev;
  int threads;
  size_t lds;
  mass_shape(dim, k, kp, A.nm, max_stack, A.cpb, threads, lds);
  const dim3 g((unsigned)((n_cells + A.cpb - 1) / A.cpb)), b((unsigned)threads);
#define GLS_MASS_MODE(D, KK, KKP, MP)                                                         \
  if (mode == kMassApply) hipLaunchKernelGGL((k_mass<D, KK, KKP, MP, kMassApply>), g, b, lds, s, A); \
  else if (mode == kMassRhs) hipLaunchKernelGGL((k_mass<D, KK, KKP, MP, kMassRhs>), g, b, lds, s, A); \
  else hipLaunchKernelGGL((k_mass<D, KK, KKP, MP, kMassDiag>), g, b, lds, s, A);
#define GLS_MASS_CASE(D, KK, KKP)           \
  if (dim == D && k == KK && kp == KKP) {   \
    if (map_degree) {                       \
      GLS_MASS_MODE(D, KK, KKP, true)       \
    } else {                                \
      GLS_MASS_MODE(D, KK, KKP, false)      \
    }                                       \
  }
  GLS_MASS_CASE(2, 1, 1)
  GLS_MASS_CASE(2, 2, 1)
  GLS_MASS_CASE(2, 2, 2)
  GLS_MASS_CASE(3, 1, 1)
  GLS_MASS_CASE(3, 2, 1)
  GLS_MASS_CASE(3, 2, 2)
#undef GLS_MASS_CASE
#undef GLS_MASS_MODE
  return hipGetLastError();
}

}  // namespace gls
