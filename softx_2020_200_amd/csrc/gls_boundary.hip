// gls_boundary.hip — forces and torques on the boundaries (the reference's calculate_forces /
// calculate_torques, postprocessing_force.cc:67-110 and postprocessing_torque.cc:67-125, restated):
// for every boundary face whose id belongs to a boundary condition (its row of the tables = `slot`),
// at the points of QGauss<dim-1> on the face,
//   n = -(outward unit normal),  sigma = nu (grad u + grad u^T) - p I,
//   f += sigma n JxW,            T += (x_q - cor) x (sigma n JxW)   (2D: T_z only).
// The reference makes one pass over the mesh per boundary condition; here every boundary goes through
// one launch (plus one finishing launch).
//
// Work decomposition: one lane per face POINT, the points of a face on consecutive lanes. The boundary
// of a mesh has few faces (a surface: ~N^(2/3) of N cells), so a lane per face would leave most of a
// small grid empty and run the nqf points of a face one after the other in each lane; a lane per point
// gives nqf times the lanes for the same registers per lane. The lanes of one face read the same node
// list and nodal values (one cell: the loads hit the same lines) and consecutive entries of the per-point
// geometry. Velocity and pressure are evaluated at the same point from the context's cell_vnodes /
// cell_pnodes; the 1D Lagrange tables and the per-lane arrays are indexed by compile-time constants only
// (loops over the nodes fully unrolled), so they stay in registers.
//
// Sums: no floating-point atomics (DESIGN row a5). Each block writes its points' six values to LDS and
// sums them per (slot, component) in lane order; the finishing kernel adds the block partials in block
// order. Two calls give bitwise identical tables.
#include "gls_launch.hpp"

namespace gls {

namespace {

constexpr int kLoadBlock = 256;

// equidistant Lagrange basis of degree M (the FE_Q(M) lattice for M <= 2) and its derivative at x
template <int M>
__device__ __forceinline__ void basis1d(double x, double (&v)[M + 1], double (&dv)[M + 1]) {
  static_assert(M == 1 || M == 2, "degrees 1 and 2");
  if constexpr (M == 1) {
    v[0] = 1.0 - x;
    v[1] = x;
    dv[0] = -1.0;
    dv[1] = 1.0;
  } else {
    v[0] = (2.0 * x - 1.0) * (x - 1.0);
    v[1] = 4.0 * x * (1.0 - x);
    v[2] = x * (2.0 * x - 1.0);
    dv[0] = 4.0 * x - 3.0;
    dv[1] = 4.0 - 8.0 * x;
    dv[2] = 4.0 * x - 1.0;
  }
}

template <int DIM, int K, int KP>
__global__ void __launch_bounds__(kLoadBlock)
    k_boundary_loads(const int32_t *__restrict__ cell_vnodes, const int32_t *__restrict__ cell_pnodes,
                     const double *__restrict__ sol, int64_t pbase, int64_t n_pts, int nqf,
                     const int32_t *__restrict__ fcell, const int32_t *__restrict__ fslot, const double *__restrict__ xi,
                     const double *__restrict__ jinv, const double *__restrict__ normal, const double *__restrict__ jxw,
                     const double *__restrict__ xq, double nu, const double *__restrict__ cor, int n_slots,
                     double *__restrict__ partial) {
  constexpr int K1 = K + 1, P1 = KP + 1;
  constexpr int NV = DIM == 3 ? K1 * K1 * K1 : K1 * K1;
  constexpr int NP = DIM == 3 ? P1 * P1 * P1 : P1 * P1;
  constexpr int NZ = DIM == 3 ? K1 : 1, PZ = DIM == 3 ? P1 : 1;
  __shared__ double sv[6][kLoadBlock + 1];  // +1: the six component rows start on different banks
  __shared__ int ss[kLoadBlock];
  const int tid = threadIdx.x;
  const int64_t pt = (int64_t)blockIdx.x * kLoadBlock + tid;
  int slot = -1;
  int64_t face = 0;
  if (pt < n_pts) {
    face = pt / nqf;
    slot = fslot[face];
  }
  double val[6] = {0, 0, 0, 0, 0, 0};  // f_x f_y f_z T_x T_y T_z
  if (slot >= 0) {
    const int64_t cell = fcell[face];
    double x[3] = {0, 0, 0}, v[3][K1], dv[3][K1];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      x[d] = xi[pt * DIM + d];
      basis1d<K>(x[d], v[d], dv[d]);
    }
    double gxi[DIM][DIM];  // d u_c / d xi_a
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int a = 0; a < DIM; ++a) gxi[c][a] = 0.0;
    const int32_t *vn = cell_vnodes + cell * NV;
#pragma unroll
    for (int az = 0; az < NZ; ++az)
#pragma unroll
      for (int ay = 0; ay < K1; ++ay)
#pragma unroll
        for (int ax = 0; ax < K1; ++ax) {
          const int64_t node = vn[ax + K1 * (ay + K1 * az)];
          double dphi[DIM];
          dphi[0] = dv[0][ax] * v[1][ay];
          dphi[1] = v[0][ax] * dv[1][ay];
          if constexpr (DIM == 3) {
            dphi[0] *= v[2][az];
            dphi[1] *= v[2][az];
            dphi[2] = v[0][ax] * v[1][ay] * dv[2][az];
          }
#pragma unroll
          for (int c = 0; c < DIM; ++c) {
            const double u = sol[node * DIM + c];
#pragma unroll
            for (int a = 0; a < DIM; ++a) gxi[c][a] += dphi[a] * u;
          }
        }
    double p = 0.0;
    {
      double w[3][P1], dw[3][P1];
#pragma unroll
      for (int d = 0; d < DIM; ++d) basis1d<KP>(x[d], w[d], dw[d]);
      const int32_t *pn = cell_pnodes + cell * NP;
#pragma unroll
      for (int az = 0; az < PZ; ++az)
#pragma unroll
        for (int ay = 0; ay < P1; ++ay)
#pragma unroll
          for (int ax = 0; ax < P1; ++ax) {
            double phi = w[0][ax] * w[1][ay];
            if constexpr (DIM == 3) phi *= w[2][az];
            p += phi * sol[pbase + pn[ax + P1 * (ay + P1 * az)]];
          }
    }
    double G[DIM][DIM];  // d u_c / d x_i = sum_a jinv[a][i] d u_c / d xi_a
    const double *ji = jinv + pt * DIM * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) s += ji[a * DIM + i] * gxi[c][a];
        G[c][i] = s;
      }
    const double w = jxw[pt];
    double f[3] = {0, 0, 0}, r[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < DIM; ++i) s += (nu * (G[c][i] + G[i][c]) - (i == c ? p : 0.0)) * -normal[pt * DIM + i];
      f[c] = s * w;
      r[c] = xq[pt * DIM + c] - cor[slot * 3 + c];
    }
    val[0] = f[0];
    val[1] = f[1];
    val[2] = f[2];
    if constexpr (DIM == 3) {
      val[3] = r[1] * f[2] - r[2] * f[1];
      val[4] = r[2] * f[0] - r[0] * f[2];
    }
    val[5] = r[0] * f[1] - r[1] * f[0];
  }
  ss[tid] = slot;
#pragma unroll
  for (int c = 0; c < 6; ++c) sv[c][tid] = val[c];
  __syncthreads();
  // fixed order: entry (slot s, component c) = the block's points of slot s in lane order
  for (int e = tid; e < n_slots * 6; e += kLoadBlock) {
    const int s = e / 6, c = e % 6;
    double acc = 0.0;
    for (int l = 0; l < kLoadBlock; ++l)
      if (ss[l] == s) acc += sv[c][l];
    partial[(int64_t)blockIdx.x * n_slots * 6 + e] = acc;
  }
}

// out[e] = sum of the block partials in block order
__global__ void __launch_bounds__(kLoadBlock) k_boundary_finish(const double *__restrict__ partial, int64_t n_blocks, int n6,
                                                                double *__restrict__ out) {
  const int e = blockIdx.x * kLoadBlock + threadIdx.x;
  if (e >= n6) return;
  double acc = 0.0;
  for (int64_t b = 0; b < n_blocks; ++b) acc += partial[b * n6 + e];
  out[e] = acc;
}

}  // namespace

int64_t boundary_loads_blocks(int64_t n_pts) { return (n_pts + kLoadBlock - 1) / kLoadBlock; }

bool boundary_loads_supported(int dim, int k, int kp) {
  return (dim == 2 || dim == 3) && ((k == 1 && kp == 1) || (k == 2 && kp == 1) || (k == 2 && kp == 2));
}

hipError_t launch_boundary_loads(int dim, int k, int kp, const int32_t *cell_vnodes, const int32_t *cell_pnodes,
                                 const double *sol, int64_t pbase, int64_t n_pts, int nqf, const int32_t *fcell,
                                 const int32_t *fslot, const double *xi, const double *jinv, const double *normal,
                                 const double *jxw, const double *xq, double nu, const double *cor, int n_slots,
                                 double *partial, double *out, hipStream_t s) {
  if (!boundary_loads_supported(dim, k, kp)) return hipErrorNotSupported;
  if (n_pts <= 0 || n_slots <= 0) return hipErrorInvalidValue;
  const int64_t nb = boundary_loads_blocks(n_pts);
  const dim3 g((unsigned)nb), b(kLoadBlock);
#define GLS_LOADS_CASE(D, KK, PP)                                                                                      \
  if (dim == D && k == KK && kp == PP)                                                                                 \
    hipLaunchKernelGGL((k_boundary_loads<D, KK, PP>), g, b, 0, s, cell_vnodes, cell_pnodes, sol, pbase, n_pts, nqf,    \
                       fcell, fslot, xi, jinv, normal, jxw, xq, nu, cor, n_slots, partial);
  GLS_LOADS_CASE(2, 1, 1)
  GLS_LOADS_CASE(2, 2, 1)
  GLS_LOADS_CASE(2, 2, 2)
  GLS_LOADS_CASE(3, 1, 1)
  GLS_LOADS_CASE(3, 2, 1)
  GLS_LOADS_CASE(3, 2, 2)
#undef GLS_LOADS_CASE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n6 = n_slots * 6;
  hipLaunchKernelGGL(k_boundary_finish, dim3((unsigned)((n6 + kLoadBlock - 1) / kLoadBlock)), b, 0, s, partial, nb, n6, out);
  return hipGetLastError();
}

}  // namespace gls
