// gls_output.hip — the point data of a VTU piece in one launch: for every cell and every patch point of
// DataOut::build_patches(mapping, subdivision) the position, velocity, pressure, vorticity, the reference's
// running-sum q_criterion and, with SRF, velocity_eulerian (navier_stokes_base.cc:1035-1064,
// post_processors.h:27-171; the host restatement is gls_vtu_write in gls_io.cpp). The arrays come out in the
// VTU layout, point P = cell * npp + p with p x-fastest over the (ns+1)^dim lattice: the host only encodes.
//
// Work decomposition: one lane per patch point, the cells packed into the block. A block takes cpb consecutive
// cells and its lane t is point p = t % npp of cell t / npp, so lane t writes point P = first_cell * npp + t:
// a wave stores 64 consecutive points of every array (scalar arrays: one 512-byte run per instruction; the
// 3-component arrays: the same 1536-byte run by three instructions issued back to back, which L2 merges into
// full lines). One lane per cell would store with stride npp and use 1/npp of every line.
//
// The evaluation is sum-factorized through LDS, the whole block sharing each sweep: the nodal values of a
// cell's fields (dim velocity components, the pressure, and for mapped cells the dim coordinates of the
// MappingQ support points) are gathered once, then
//   A: x sweep, (t0, a1, a2) <- sum_a0 {V, D}[t0][a0] f[a0, a1, a2]
//   B: y sweep (3D), (t0, t1, a2) <- sum_a1 of {V A_v, V A_d, D A_v}
// and each lane finishes its own point with the last direction in registers (value and dim derivatives by
// 4 (k+1) FMAs per field in 3D where the dense contraction takes 4 (k+1)^3). The sweeps' items are dealt to
// all lanes of the block, whichever cell they belong to. Patch points are not quadrature points, so the
// geometry is the plan's: box cells x = x0 + h t / ns (the host's expression: bitwise the host's points) and
// grad = grad_ref / h; mapped cells x, J = d x / d xi from the support points as one more set of fields, J^-1
// by cofactors as on the host.
//
// q_criterion: the reference keeps its two accumulators across the points of a patch, so the value at point p
// is 0.5 (sum_{p' <= p} |W|^2 - sum_{p' <= p} |S|^2), restarted at every cell. Each lane leaves its point's
// |W|^2 and |S|^2 in LDS and then adds up its own cell's entries 0..p in patch order: the two sums stay apart
// and are subtracted last, the order is the host's, and a cell whose lanes straddle two waves (npp does not
// divide 64) needs no special case. The loop reads the same LDS word in all lanes of a cell (a broadcast) and
// is npp / 2 steps on average, at most 256: small next to the stores that bound the kernel.
//
// No atomics, every sum in a fixed order: two calls on the same input are bitwise equal, and a context's
// layout (brick, per cell, mapped, hanging lines) enters only through cell_vnodes / cell_pnodes.
// Instantiated for dim 2, 3 x (k, kp) in {(1,1), (2,1), (2,2)} x box / mapped; the subdivision and the
// mapping degree are run-time values (npp <= 256: subdivision <= 15 in 2D, <= 5 in 3D).
#include "gls_launch.hpp"
#include "gls_lattice_eval.hpp"  // the sweeps and the field layout, shared with gls_error.hip

namespace gls {

namespace {

constexpr int kOutMaxBlock = 256;                 // lanes per block at most = patch points per cell at most
constexpr int kOutLdsDoubles = 48 * 1024 / 8;     // LDS budget of one block

struct OutputArgs {
  const int32_t *cell_vnodes, *cell_pnodes;
  const double *sol;
  int64_t pbase;          // the pressure of node n is sol[pbase + n]
  const double *x0h;      // box cells: [n_cells][2 dim] = x0 | h
  const double *support;  // mapped cells: [n_cells][nm^dim][dim]
  const double *tab;      // Vv [np1][k+1] | Dv | Vp [np1][kp+1] | Vm [np1][nm] | Dm
  int64_t n_cells;
  int ns, nm, cpb;
  int srf;
  double omega[3];
  double *pts, *vel, *pre, *vort, *qcr, *eul;
};

template <int DIM, int K, int KP, bool MAPPED>
__global__ void __launch_bounds__(kOutMaxBlock) k_output_fields(const OutputArgs A) {
  constexpr int K1 = K + 1, KP1 = KP + 1, NV = opow(K1, DIM), NP = opow(KP1, DIM);
  extern __shared__ double lds[];
  const int ns = A.ns, np1 = ns + 1, npp = opow(np1, DIM), nm = A.nm, nsup = opow(nm, DIM);
  const int tid = threadIdx.x, nthr = blockDim.x;
  // LDS: tables | |W|^2 [nthr] | |S|^2 [nthr] | per cell: velocity fields, pressure, support coordinates
  const int ntab = np1 * (2 * K1 + KP1 + (MAPPED ? 2 * nm : 0));
  double *tVv = lds, *tDv = tVv + np1 * K1, *tVp = tDv + np1 * K1, *tVm = tVp + np1 * KP1, *tDm = tVm + np1 * nm;
  double *lw = lds + ntab, *lsq = lw + nthr, *cells = lsq + nthr;
  const int fv = field_doubles(DIM, K1, np1, true), fp = field_doubles(DIM, KP1, np1, false),
            fm = MAPPED ? field_doubles(DIM, nm, np1, true) : 0;
  const int off_p = DIM * fv, off_m = off_p + fp, cs = off_m + DIM * fm;
  const int64_t cell0 = (int64_t)blockIdx.x * A.cpb;
  const int ncl = (int)(A.n_cells - cell0 < A.cpb ? A.n_cells - cell0 : A.cpb);

  for (int i = tid; i < ntab; i += nthr) lds[i] = A.tab[i];
  // gather: velocity [cl][a][c] (the components of a node are adjacent in sol), pressure, support points
  for (int i = tid; i < ncl * NV * DIM; i += nthr) {
    const int cl = i / (NV * DIM), r = i - cl * (NV * DIM), a = r / DIM, c = r - a * DIM;
    const int64_t node = A.cell_vnodes[(cell0 + cl) * NV + a];
    cells[cl * cs + c * fv + a] = A.sol[node * DIM + c];
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
#pragma unroll
  for (int c = 0; c < DIM; ++c) sweep_a<DIM, true>(cells + c * fv, cs, ncl, K1, np1, tVv, tDv);
  sweep_a<DIM, false>(cells + off_p, cs, ncl, KP1, np1, tVp, nullptr);
  if constexpr (MAPPED) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_a<DIM, true>(cells + off_m + c * fm, cs, ncl, nm, np1, tVm, tDm);
  }
  __syncthreads();
  if constexpr (DIM == 3) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) sweep_b<true>(cells + c * fv, cs, ncl, K1, np1, tVv, tDv);
    sweep_b<false>(cells + off_p, cs, ncl, KP1, np1, tVp, nullptr);
    if constexpr (MAPPED) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) sweep_b<true>(cells + off_m + c * fm, cs, ncl, nm, np1, tVm, tDm);
    }
    __syncthreads();
  }

  const bool active = tid < ncl * npp;
  const int cl = active ? tid / npp : 0, p = active ? tid - cl * npp : 0;
  const int tt[3] = {p % np1, (p / np1) % np1, DIM == 3 ? p / (np1 * np1) : 0};
  const int64_t cell = cell0 + cl, P = cell0 * npp + tid;
  double u[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0}, G[3][3], pv = 0.0, w2 = 0.0, s2 = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 3; ++i) G[c][i] = 0.0;
  if (active) {
    const double *cf = cells + cl * cs;
    double gx[3][3], dummy[3];  // gx[c][a] = d u_c / d xi_a
#pragma unroll
    for (int c = 0; c < DIM; ++c) finish<DIM, true>(cf + c * fv, K1, np1, tt, tVv, tDv, u[c], gx[c]);
    finish<DIM, false>(cf + off_p, KP1, np1, tt, tVp, nullptr, pv, dummy);
    if constexpr (MAPPED) {
      double J[3][3], JI[3][3];  // J[i][a] = d x_i / d xi_a, JI[a][i] = d xi_a / d x_i
#pragma unroll
      for (int i = 0; i < DIM; ++i) finish<DIM, true>(cf + off_m + i * fm, nm, np1, tt, tVm, tDm, x[i], J[i]);
      if constexpr (DIM == 2) {
        const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        JI[0][0] = J[1][1] / det;
        JI[0][1] = -J[0][1] / det;
        JI[1][0] = -J[1][0] / det;
        JI[1][1] = J[0][0] / det;
      } else {
        const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                           J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int i = 0; i < 3; ++i)
            JI[a][i] = (J[(i + 1) % 3][(a + 1) % 3] * J[(i + 2) % 3][(a + 2) % 3] -
                        J[(i + 1) % 3][(a + 2) % 3] * J[(i + 2) % 3][(a + 1) % 3]) / det;
      }
#pragma unroll
      for (int c = 0; c < DIM; ++c)
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < DIM; ++a) s += JI[a][i] * gx[c][a];
          G[c][i] = s;
        }
    } else {
      const double *xh = A.x0h + cell * 2 * DIM;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        const double h = xh[DIM + d];
        x[d] = xh[d] + h * tt[d] / ns;
#pragma unroll
        for (int c = 0; c < DIM; ++c) G[c][d] = gx[c][d] / h;
      }
    }
#pragma unroll
    for (int j = 0; j < DIM; ++j)
#pragma unroll
      for (int e = 0; e < DIM; ++e) {
        const double W = 0.5 * (G[j][e] - G[e][j]), S = 0.5 * (G[j][e] + G[e][j]);
        w2 += W * W;
        s2 += S * S;
      }
  }
  lw[tid] = w2;
  lsq[tid] = s2;
  __syncthreads();
  if (!active) return;
  double p1 = 0.0, r1 = 0.0;  // the reference's accumulators, restarted at the cell's first point
  for (int i = tid - p; i <= tid; ++i) {
    p1 += lw[i];
    r1 += lsq[i];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    A.pts[3 * P + d] = x[d];
    A.vel[3 * P + d] = u[d];
  }
  A.pre[P] = pv;
  if constexpr (DIM == 3) {  // post_processors.h:41-50
    A.vort[3 * P + 0] = G[2][1] - G[1][2];
    A.vort[3 * P + 1] = G[0][2] - G[2][0];
    A.vort[3 * P + 2] = G[1][0] - G[0][1];
  } else {
    A.vort[P] = G[1][0] - G[0][1];
  }
  A.qcr[P] = 0.5 * (p1 - r1);
  if (A.srf) {  // post_processors.h:138-160: u + Omega x x
    const double *o = A.omega;
    if constexpr (DIM == 3) {
      A.eul[3 * P + 0] = u[0] + o[1] * x[2] - o[2] * x[1];
      A.eul[3 * P + 1] = u[1] + o[2] * x[0] - o[0] * x[2];
      A.eul[3 * P + 2] = u[2] + o[0] * x[1] - o[1] * x[0];
    } else {
      A.eul[3 * P + 0] = u[0] - o[2] * x[1];
      A.eul[3 * P + 1] = u[1] + o[2] * x[0];
      A.eul[3 * P + 2] = 0.0;
    }
  }
}

// cells per block and lanes per block for this element and subdivision; false: no launch shape exists
bool output_shape(int dim, int k, int kp, int nm, int ns, int &cpb, int &threads, size_t &lds_bytes) {
  const int np1 = ns + 1, npp = opow(np1, dim);
  if (npp > kOutMaxBlock) return false;
  const int per_cell = dim * field_doubles(dim, k + 1, np1, true) + field_doubles(dim, kp + 1, np1, false) +
                       (nm ? dim * field_doubles(dim, nm, np1, true) : 0);
  const int fixed = np1 * (2 * (k + 1) + (kp + 1) + 2 * nm) + 2 * kOutMaxBlock;
  if (fixed + per_cell > kOutLdsDoubles) return false;
  cpb = std::min(kOutMaxBlock / npp, (kOutLdsDoubles - fixed) / per_cell);
  threads = (cpb * npp + 63) / 64 * 64;
  lds_bytes = sizeof(double) * (size_t)(fixed - 2 * kOutMaxBlock + 2 * threads + cpb * per_cell);
  return true;
}

}  // namespace

bool output_fields_supported(int dim, int k, int kp, int map_degree, int subdivision) {
  int cpb, threads;
  size_t lds;
  return (dim == 2 || dim == 3) && ((k == 1 && kp == 1) || (k == 2 && kp == 1) || (k == 2 && kp == 2)) &&
         map_degree >= 0 && map_degree <= 3 && subdivision >= 1 &&
         output_shape(dim, k, kp, map_degree ? map_degree + 1 : 0, subdivision, cpb, threads, lds);
}

hipError_t launch_output_fields(int dim, int k, int kp, int map_degree, int subdivision, const int32_t *cell_vnodes,
                                const int32_t *cell_pnodes, const double *sol, int64_t pbase, const double *x0h,
                                const double *support, const double *tab, int64_t n_cells, int srf, const double *omega,
                                double *pts, double *vel, double *pre, double *vort, double *qcr, double *eul,
                                hipStream_t s) {
  if (!output_fields_supported(dim, k, kp, map_degree, subdivision)) return hipErrorNotSupported;
  if (n_cells <= 0 || (map_degree ? !support : !x0h) || (srf && !eul)) return hipErrorInvalidValue;
  OutputArgs A;
  A.cell_vnodes = cell_vnodes;
  A.cell_pnodes = cell_pnodes;
  A.sol = sol;
  A.pbase = pbase;
  A.x0h = x0h;
  A.support = support;
  A.tab = tab;
  A.n_cells = n_cells;
  A.ns = subdivision;
  A.nm = map_degree ? map_degree + 1 : 0;
  A.srf = srf;
  for (int i = 0; i < 3; ++i) A.omega[i] = omega ? omega[i] : 0.0;
  A.pts = pts;
  A.vel = vel;
  A.pre = pre;
  A.vort = vort;
  A.qcr = qcr;
  A.eul = eul;
  int threads;
  size_t lds;
  output_shape(dim, k, kp, A.nm, subdivision, A.cpb, threads, lds);
  const dim3 g((unsigned)((n_cells + A.cpb - 1) / A.cpb)), b((unsigned)threads);
#define GLS_OUT_CASE(D, KK, KKP)                                                                  \
  if (dim == D && k == KK && kp == KKP) {                                                         \
    if (map_degree)                                                                               \
      hipLaunchKernelGGL((k_output_fields<D, KK, KKP, true>), g, b, lds, s, A);                   \
    else                                                                                          \
      hipLaunchKernelGGL((k_output_fields<D, KK, KKP, false>), g, b, lds, s, A);                  \
  }
  GLS_OUT_CASE(2, 1, 1)
  GLS_OUT_CASE(2, 2, 1)
  GLS_OUT_CASE(2, 2, 2)
  GLS_OUT_CASE(3, 1, 1)
  GLS_OUT_CASE(3, 2, 1)
  GLS_OUT_CASE(3, 2, 2)
#undef GLS_OUT_CASE
  return hipGetLastError();
}

}  // namespace gls
