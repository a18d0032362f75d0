// gls_diagnostics.hip — flow diagnostics of a solution vector in one pass over the cells: the CFL number
// (the reference's calculate_CFL, postprocessing_cfl.cc:36-87, restated: |u| at the reference cell's centre
// times dt / h, h = sqrt(4|K|/pi)/deg in 2D, (6|K|/pi)^(1/3)/deg in 3D), the kinetic energy integral
// int 1/2 |u|^2 (postprocessing_kinetic_energy.cc), the enstrophy integral int 1/2 |curl u|^2
// (postprocessing_enstrophy.cc; 2D: omega_z) and the volume sum JxW, the last three with the context's
// QGauss(k+1).
//
// Work decomposition: one lane per cell. The pass reads each cell's nodal velocities once (the (k+1)^dim x dim
// values stay in registers: every loop over the nodes is fully unrolled, so the arrays are indexed by
// compile-time constants only) and walks the quadrature points in a run-time loop; the 1D tables are read
// through a uniform index (scalar loads). Box cells take grad u = grad_ref u / h and JxW = w h_x h_y h_z
// from the cell extents, mapped cells J^-1 and JxW from the context's per-point geometry. Only the velocity
// enters, so one instantiation per (dim, k) serves every pressure degree. The pass moves ~ (k+1)^dim (dim
// doubles + an index) per cell plus the mapped geometry: bandwidth-trivial next to a Newton step.
//
// Reduction: no atomics (DESIGN row a5). Each block folds its lanes' four values in LDS (a halving tree: a
// fixed order) into partial[block][4]; one finishing block then gives each lane the partials block = lane,
// lane + 256, ... in ascending order and folds the lanes with the same tree. Two calls on the same input
// give bitwise identical results.
#include "gls_launch.hpp"

namespace gls {

namespace {

constexpr int kDiagBlock = 256;  // 4 wave64 per block

// fold the block's four values (max, sum, sum, sum) into lane 0; red: [4][kDiagBlock]
__device__ __forceinline__ void block_fold(double (&v)[4], double (*red)[kDiagBlock]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) red[i][tid] = v[i];
  __syncthreads();
  for (int st = kDiagBlock / 2; st > 0; st >>= 1) {
    if (tid < st) {
      red[0][tid] = fmax(red[0][tid], red[0][tid + st]);
#pragma unroll
      for (int i = 1; i < 4; ++i) red[i][tid] += red[i][tid + st];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = red[i][0];
}

// tab: V [NQ1][K1] | D [NQ1][K1] | w [NQ1] (velocity basis values / derivatives at the 1D Gauss points)
template <int DIM, int K, bool GEN>
__global__ void __launch_bounds__(kDiagBlock)
    k_flow_diagnostics(const int32_t *__restrict__ cell_vnodes, const double *__restrict__ geo,
                       const double *__restrict__ gq, const double *__restrict__ meas, const double *__restrict__ tab,
                       const double *__restrict__ sol, int64_t n_cells, double dt, double *__restrict__ partial) {
  constexpr int K1 = K + 1, NQ1 = K + 1;
  constexpr int NV = DIM == 3 ? K1 * K1 * K1 : K1 * K1;
  constexpr int NQ = DIM == 3 ? NQ1 * NQ1 * NQ1 : NQ1 * NQ1;
  constexpr int NZ = DIM == 3 ? K1 : 1;
  __shared__ double red[4][kDiagBlock];
  const double *tV = tab, *tD = tab + NQ1 * K1, *tW = tab + 2 * NQ1 * K1;
  const int64_t cell = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
  double val[4] = {0.0, 0.0, 0.0, 0.0};  // CFL, int 1/2 |u|^2, int 1/2 |curl u|^2, volume
  if (cell < n_cells) {
    double u[NV][DIM];
    const int32_t *vn = cell_vnodes + cell * NV;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
      const int64_t node = vn[a];
#pragma unroll
      for (int c = 0; c < DIM; ++c) u[a][c] = sol[node * DIM + c];
    }
    // CFL: the velocity at the reference cell's centre (QGauss(1))
    {
      double B[K1];
      if constexpr (K == 1) {
        B[0] = 0.5;
        B[1] = 0.5;
      } else {
        B[0] = 0.0;
        B[1] = 1.0;
        B[2] = 0.0;
      }
      double uc[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) uc[c] = 0.0;
#pragma unroll
      for (int az = 0; az < NZ; ++az)
#pragma unroll
        for (int ay = 0; ay < K1; ++ay)
#pragma unroll
          for (int ax = 0; ax < K1; ++ax) {
            const double w = B[ax] * B[ay] * (DIM == 3 ? B[az] : 1.0);
#pragma unroll
            for (int c = 0; c < DIM; ++c) uc[c] += w * u[ax + K1 * (ay + K1 * az)][c];
          }
      const double m = meas[cell], deg = (double)K;  // deg = max(k, kp) = k
      const double hh = DIM == 2 ? sqrt(4. * m / M_PI) / deg : cbrt(6. * m / M_PI) / deg;
      double un = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) un += uc[c] * uc[c];
      val[0] = sqrt(un) / hh * dt;
    }
    const double hx = geo[cell * 4 + 0], hy = geo[cell * 4 + 1], hz = DIM == 3 ? geo[cell * 4 + 2] : 1.0;
    const double ih[3] = {1.0 / hx, 1.0 / hy, 1.0 / hz};
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
      const int qx = q % NQ1, qy = (q / NQ1) % NQ1, qz = DIM == 3 ? q / (NQ1 * NQ1) : 0;
      double uq[DIM], gxi[DIM][DIM];  // u_c, d u_c / d xi_a
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        uq[c] = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) gxi[c][a] = 0.0;
      }
#pragma unroll
      for (int az = 0; az < NZ; ++az)
#pragma unroll
        for (int ay = 0; ay < K1; ++ay)
#pragma unroll
          for (int ax = 0; ax < K1; ++ax) {
            const double vx = tV[qx * K1 + ax], vy = tV[qy * K1 + ay], vz = DIM == 3 ? tV[qz * K1 + az] : 1.0;
            const double phi = vx * vy * vz;
            double dphi[DIM];
            dphi[0] = tD[qx * K1 + ax] * vy * vz;
            dphi[1] = vx * tD[qy * K1 + ay] * vz;
            if constexpr (DIM == 3) dphi[2] = vx * vy * tD[qz * K1 + az];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
              const double un = u[ax + K1 * (ay + K1 * az)][c];
              uq[c] += phi * un;
#pragma unroll
              for (int a = 0; a < DIM; ++a) gxi[c][a] += dphi[a] * un;
            }
          }
      double G[DIM][DIM], JxW;  // d u_c / d x_i
      if constexpr (GEN) {
        const double *g = gq + (cell * NQ + q) * kGeo;
        JxW = g[kGeoJxW];
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
          for (int i = 0; i < DIM; ++i) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) s += g[kGeoJI + 3 * a + i] * gxi[c][a];
            G[c][i] = s;
          }
      } else {
        JxW = tW[qx] * tW[qy] * (DIM == 3 ? tW[qz] : 1.0) * hx * hy * (DIM == 3 ? hz : 1.0);
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
          for (int i = 0; i < DIM; ++i) G[c][i] = gxi[c][i] * ih[i];
      }
      double ke = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) ke += uq[c] * uq[c];
      const double wz = G[1][0] - G[0][1];
      double en = wz * wz;
      if constexpr (DIM == 3) {
        const double wx = G[2][1] - G[1][2], wy = G[0][2] - G[2][0];
        en += wx * wx + wy * wy;
      }
      val[1] += 0.5 * ke * JxW;
      val[2] += 0.5 * en * JxW;
      val[3] += JxW;
    }
  }
  block_fold(val, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) partial[(int64_t)blockIdx.x * 4 + i] = val[i];
  }
}

// out[4] = the block partials folded: lane l takes blocks l, l + 256, ... in ascending order
__global__ void __launch_bounds__(kDiagBlock)
    k_flow_diagnostics_finish(const double *__restrict__ partial, int64_t n_blocks, double *__restrict__ out) {
  __shared__ double red[4][kDiagBlock];
  double val[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < n_blocks; b += kDiagBlock) {
    val[0] = fmax(val[0], partial[b * 4]);
#pragma unroll
    for (int i = 1; i < 4; ++i) val[i] += partial[b * 4 + i];
  }
  block_fold(val, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = val[i];
  }
}

}  // namespace

int64_t flow_diagnostics_blocks(int64_t n_cells) { return (n_cells + kDiagBlock - 1) / kDiagBlock; }

bool flow_diagnostics_supported(int dim, int k, int kp) {
  return (dim == 2 || dim == 3) && ((k == 1 && kp == 1) || (k == 2 && kp == 1) || (k == 2 && kp == 2));
}

hipError_t launch_flow_diagnostics(int dim, int k, const int32_t *cell_vnodes, const double *geo, const double *gq,
                                   const double *meas, const double *tab, const double *sol, int64_t n_cells, double dt,
                                   double *partial, double *out, hipStream_t s) {
  if ((dim != 2 && dim != 3) || (k != 1 && k != 2)) return hipErrorNotSupported;
  if (n_cells <= 0) return hipErrorInvalidValue;
  const int64_t nb = flow_diagnostics_blocks(n_cells);
  const dim3 g((unsigned)nb), b(kDiagBlock);
#define GLS_DIAG_CASE(D, KK)                                                                                         \
  if (dim == D && k == KK) {                                                                                         \
    if (gq)                                                                                                          \
      hipLaunchKernelGGL((k_flow_diagnostics<D, KK, true>), g, b, 0, s, cell_vnodes, geo, gq, meas, tab, sol, n_cells, \
                         dt, partial);                                                                               \
    else                                                                                                             \
      hipLaunchKernelGGL((k_flow_diagnostics<D, KK, false>), g, b, 0, s, cell_vnodes, geo, gq, meas, tab, sol,       \
                         n_cells, dt, partial);                                                                      \
  }
  GLS_DIAG_CASE(2, 1)
  GLS_DIAG_CASE(2, 2)
  GLS_DIAG_CASE(3, 1)
  GLS_DIAG_CASE(3, 2)
#undef GLS_DIAG_CASE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_flow_diagnostics_finish, dim3(1), b, 0, s, partial, nb, out);
  return hipGetLastError();
}

}  // namespace gls
