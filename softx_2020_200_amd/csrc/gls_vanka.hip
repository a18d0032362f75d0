// gls_vanka.hip — the additive cell-Vanka smoother of the hierarchy multigrid for 3D Q2-Qk' cells (k' = 1, 2; mapped or
// axis-aligned), matrix-free up to the cell patches:
//   x <- x + omega D_m^-1 sum_c R_c^T A_c^-1 R_c (b - A x),   A_c = R_c A R_c^T (nd x nd, nd = 89 / 108).
// Setup, once per Jacobian state (gls_vanka_host.cpp):
//   k_vanka_element : K_c, the per-cell J.v's pointwise algebra (gls_cell_point.hpp, from the linearization cache)
//                     applied to the nd unit vectors; one workgroup per cell, 9 columns x 27 quadrature points at a time
//                     through LDS, FP64
//   k_vanka_patch   : A_c = sum over the neighbour cells c' (ascending) of the entries of K_c' whose row and column DoF
//                     both lie in c (host-built overlap maps); constrained DoFs become identity rows / columns scaled by
//                     the diagonal kernel's value
//   k_vanka_invert  : Gauss-Jordan with partial pivoting in LDS, FP64, one workgroup per cell (nd x (nd | 1) doubles:
//                     63 / 94 KB); the inverse stored FP32 row-major, rows padded to 16 bytes; a zero or non-finite
//                     pivot or a non-finite inverse sets the cell's flag
// Sweep:
//   k_vanka_apply   : one wave per cell; r_c gathered into LDS (FP32), each lane streams its rows of A_c^-1 with
//                     16-byte loads and accumulates in FP32; the cell's correction as an element vector
//   k_vanka_update  : x[dof] += omega / multiplicity * (the DoF's slots summed in ascending cell order), FP64
// No floating-point atomics; every sum has a fixed order: bitwise repeatable.
#include "gls_brick_common.hpp"
#include "gls_cell_point.hpp"
#include "gls_launch.hpp"

#include <cfloat>

namespace gls {
namespace {

constexpr int kVkCols = 9;  // unit vectors per pass of the element-matrix kernel (9 x 27 points = 243 lanes)

template <int KP, bool GEN>
__global__ void __launch_bounds__(256) k_vanka_element(const OpParams P, const Tables1D T, double *__restrict__ K) {
  constexpr int NV = 27, NQ = 27, NP = (KP + 1) * (KP + 1) * (KP + 1), ND = NV * 3 + NP;
  __shared__ double sTab[3][3][3], sW[3];        // [V, D, S][q][node]
  __shared__ double sVp[3][KP + 1], sDp[3][KP + 1];
  __shared__ double sN[4][NV][NQ];               // velocity basis: value, d/dxi_0..2 at (node, point)
  __shared__ double sNp[4][NP][NQ];              // pressure basis
  __shared__ double sT[kVkCols][16][NQ];         // test coefficients of the pass's unit vectors
  const int tid = threadIdx.x;
  const int64_t cell = blockIdx.x;
  if (tid < 9) {
    const int q = tid / 3, a = tid % 3;
    sTab[0][q][a] = T.V[q][a];
    sTab[1][q][a] = T.D[q][a];
    sTab[2][q][a] = T.S[q][a];
    if (a == 0) sW[q] = T.w[q];
  }
  if (tid < 3 * (KP + 1)) {
    const int q = tid / (KP + 1), a = tid % (KP + 1);
    sVp[q][a] = T.Vp[q][a];
    sDp[q][a] = T.Dp[q][a];
  }
  __syncthreads();
  for (int t = tid; t < NV * NQ; t += 256) {
    const int a = t / NQ, q = t % NQ;
    const int ax = a % 3, ay = (a / 3) % 3, az = a / 9, qx = q % 3, qy = (q / 3) % 3, qz = q / 9;
    const double vx = sTab[0][qx][ax], vy = sTab[0][qy][ay], vz = sTab[0][qz][az];
    sN[0][a][q] = vx * vy * vz;
    sN[1][a][q] = sTab[1][qx][ax] * vy * vz;
    sN[2][a][q] = vx * sTab[1][qy][ay] * vz;
    sN[3][a][q] = vx * vy * sTab[1][qz][az];
  }
  for (int t = tid; t < NP * NQ; t += 256) {
    const int b = t / NQ, q = t % NQ;
    const int bx = b % (KP + 1), by = (b / (KP + 1)) % (KP + 1), bz = b / ((KP + 1) * (KP + 1));
    const int qx = q % 3, qy = (q / 3) % 3, qz = q / 9;
    const double vx = sVp[qx][bx], vy = sVp[qy][by], vz = sVp[qz][bz];
    sNp[0][b][q] = vx * vy * vz;
    sNp[1][b][q] = sDp[qx][bx] * vy * vz;
    sNp[2][b][q] = vx * sDp[qy][by] * vz;
    sNp[3][b][q] = vx * vy * sDp[qz][bz];
  }
  __syncthreads();
  double *Kc = K + cell * (int64_t)(ND * ND);
  for (int col0 = 0; col0 < ND; col0 += kVkCols) {
    // ---- pointwise: lane = (unit vector of the pass, quadrature point)
    if (tid < kVkCols * NQ) {
      const int cl = tid / NQ, q = tid % NQ, col = col0 + cl;
      if (col < ND) {
        const int i = q % 3, j = (q / 3) % 3, k = q / 9;
        double v[3] = {0., 0., 0.}, gv[3][3], H[3][6], vp = 0., gvp[3] = {0., 0., 0.}, tc[16];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int e = 0; e < 3; ++e) gv[c][e] = 0.;
#pragma unroll
          for (int e = 0; e < 6; ++e) H[c][e] = 0.;
        }
        if (col < NV * 3) {
          const int a = col / 3, c0 = col % 3;
          const int ax = a % 3, ay = (a / 3) % 3, az = a / 9;
          const double vx = sTab[0][i][ax], vy = sTab[0][j][ay], vz = sTab[0][k][az];
          const double dx = sTab[1][i][ax], dy = sTab[1][j][ay], dz = sTab[1][k][az];
          const double hv[6] = {sTab[2][i][ax] * vy * vz, vx * sTab[2][j][ay] * vz, vx * vy * sTab[2][k][az],
                                dx * dy * vz, dx * vy * dz, vx * dy * dz};
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double on = c == c0 ? 1.0 : 0.0;
            v[c] = on * vx * vy * vz;
            gv[c][0] = on * dx * vy * vz;
            gv[c][1] = on * vx * dy * vz;
            gv[c][2] = on * vx * vy * dz;
#pragma unroll
            for (int e = 0; e < 6; ++e) H[c][e] = on * hv[e];
          }
        } else {
          const int b = col - NV * 3;
          vp = sNp[0][b][q];
          gvp[0] = sNp[1][b][q];
          gvp[1] = sNp[2][b][q];
          gvp[2] = sNp[3][b][q];
        }
        jv_point<GEN>(P, cell, q, i, j, k, sW, v, gv, H, vp, gvp, tc);
#pragma unroll
        for (int t = 0; t < 16; ++t) sT[cl][t][q] = tc[t];
      }
    }
    __syncthreads();
    // ---- integrate against the nd test functions: item = (row, unit vector of the pass); points in ascending order
    const int ncol = ND - col0 < kVkCols ? ND - col0 : kVkCols;
    for (int t = tid; t < ND * kVkCols; t += 256) {
      const int r = t / kVkCols, cl = t % kVkCols;
      if (cl >= ncol) continue;
      const double *N0, *N1, *N2, *N3, *Tt;
      if (r < NV * 3) {
        const int a = r / 3, c = r % 3;
        N0 = sN[0][a], N1 = sN[1][a], N2 = sN[2][a], N3 = sN[3][a];
        Tt = &sT[cl][4 * c][0];
      } else {
        const int b = r - NV * 3;
        N0 = sNp[0][b], N1 = sNp[1][b], N2 = sNp[2][b], N3 = sNp[3][b];
        Tt = &sT[cl][12][0];
      }
      double acc = 0.;
      for (int q = 0; q < NQ; ++q)
        acc += N0[q] * Tt[q] + N1[q] * Tt[NQ + q] + N2[q] * Tt[2 * NQ + q] + N3[q] * Tt[3 * NQ + q];
      Kc[r * ND + col0 + cl] = acc;
    }
    __syncthreads();
  }
}

// A_c from the neighbours' element matrices; every thread owns entries of A_c and adds its neighbours in list order
__global__ void __launch_bounds__(256) k_vanka_patch(int nd, const double *__restrict__ K, const int64_t *__restrict__ nb_off,
                                                     const int32_t *__restrict__ nb_cell, const int64_t *__restrict__ ov_off,
                                                     const uint8_t *__restrict__ ov_i, const uint8_t *__restrict__ ov_j,
                                                     const int32_t *__restrict__ cell_dofs, const uint8_t *__restrict__ con,
                                                     const double *__restrict__ diag, double *__restrict__ A) {
  __shared__ int16_t loc[256];   // local index in the neighbour of c's local DoF, -1: not shared
  __shared__ uint8_t scon[256];
  const int tid = threadIdx.x;
  const int64_t cell = blockIdx.x;
  const int64_t nn = (int64_t)nd * nd;
  double *Ac = A + cell * nn;
  for (int t = tid; t < nd * nd; t += 256) Ac[t] = 0.;
  if (tid < nd) scon[tid] = con[cell_dofs[cell * nd + tid]];
  for (int64_t pr = nb_off[cell]; pr < nb_off[cell + 1]; ++pr) {
    loc[tid] = -1;
    __syncthreads();
    for (int64_t e = ov_off[pr] + tid; e < ov_off[pr + 1]; e += 256) loc[ov_i[e]] = (int16_t)ov_j[e];
    __syncthreads();
    const double *Kn = K + (int64_t)nb_cell[pr] * nn;
    for (int t = tid; t < nd * nd; t += 256) {
      const int i = t / nd, j = t - i * nd;
      const int li = loc[i], lj = loc[j];
      if (li >= 0 && lj >= 0) Ac[t] += Kn[li * nd + lj];
    }
    __syncthreads();
  }
  __syncthreads();
  for (int t = tid; t < nd * nd; t += 256) {
    const int i = t / nd, j = t - i * nd;
    if (scon[i] || scon[j]) Ac[t] = i == j ? diag[cell_dofs[cell * nd + i]] : 0.;
  }
}

// in-place Gauss-Jordan inverse with partial pivoting (the first row of the largest magnitude), FP64 in LDS
template <int ND>
__global__ void __launch_bounds__(256) k_vanka_invert(const double *__restrict__ A, float *__restrict__ Ainv, int ldi,
                                                      int32_t *__restrict__ flag) {
  constexpr int LD = ND | 1;  // odd row stride: conflict-free column walks
  __shared__ double sA[ND * LD];
  __shared__ double sRow[ND], sCol[ND];
  __shared__ int sPiv[ND];
  __shared__ int sBad;
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int64_t cell = blockIdx.x;
  const double *Ac = A + cell * (int64_t)(ND * ND);
  for (int t = tid; t < ND * ND; t += 256) sA[(t / ND) * LD + t % ND] = Ac[t];
  if (tid == 0) sBad = 0;
  __syncthreads();
  for (int p = 0; p < ND; ++p) {
    if (tid < 64) {  // pivot search by the first wave: largest |A[r][p]|, r >= p, lowest r among equals
      double best = -1.;
      int br = ND;
      bool nan = false;
      for (int r = p + tid; r < ND; r += 64) {
        const double a = fabs(sA[r * LD + p]);
        nan = nan || !(a == a);
        if (a > best) { best = a; br = r; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int orr = __shfl_xor(br, o);
        const int on = __shfl_xor((int)nan, o);
        nan = nan || on;
        if (ob > best || (ob == best && orr < br)) { best = ob; br = orr; }
      }
      if (tid == 0) {
        sPiv[p] = br < ND ? br : p;
        if (nan || !(best > DBL_MIN) || !(best <= DBL_MAX)) sBad = 1;
      }
    }
    __syncthreads();
    if (sBad) break;  // uniform: read from LDS after the barrier
    const int pr = sPiv[p];
    if (pr != p)
      for (int j = tid; j < ND; j += 256) {
        const double a = sA[p * LD + j];
        sA[p * LD + j] = sA[pr * LD + j];
        sA[pr * LD + j] = a;
      }
    __syncthreads();
    const double pinv = 1.0 / sA[p * LD + p];
    if (tid < ND) sRow[tid] = tid == p ? pinv : sA[p * LD + tid] * pinv;
    else if (tid >= 128 && tid - 128 < ND) sCol[tid - 128] = sA[(tid - 128) * LD + p];
    __syncthreads();
    for (int i = ti; i < ND; i += 16) {
      const double f = sCol[i];
      for (int j = tj; j < ND; j += 16) {
        double a;
        if (i == p) a = sRow[j];
        else if (j == p) a = -f * pinv;
        else a = sA[i * LD + j] - f * sRow[j];
        sA[i * LD + j] = a;
      }
    }
    __syncthreads();
  }
  float *out = Ainv + cell * (int64_t)ND * ldi;
  if (sBad) {
    if (tid == 0) flag[cell] = 1;
    for (int t = tid; t < ND * ldi; t += 256) out[t] = 0.f;
    return;
  }
  // the row swaps of A are column swaps of the inverse, undone in reverse order
  for (int p = ND - 1; p >= 0; --p) {
    const int pr = sPiv[p];
    if (pr != p)
      for (int i = tid; i < ND; i += 256) {
        const double a = sA[i * LD + p];
        sA[i * LD + p] = sA[i * LD + pr];
        sA[i * LD + pr] = a;
      }
    __syncthreads();
  }
  int bad = 0;
  for (int t = tid; t < ND * ldi; t += 256) {
    const int i = t / ldi, j = t - i * ldi;
    const float a = j < ND ? (float)sA[i * LD + j] : 0.f;
    bad |= !(fabsf(a) <= FLT_MAX);
    out[t] = a;
  }
  if (bad) flag[cell] = 1;  // (every writer stores the same value)
}

// one wave per cell: e_c = A_c^-1 r_c in FP32, lane = rows lane, lane + 64
template <int ND>
__global__ void __launch_bounds__(64) k_vanka_apply(int n_cells, const float *__restrict__ Ainv, int ldi,
                                                    const int32_t *__restrict__ cell_dofs, const double *__restrict__ r,
                                                    double *__restrict__ ev) {
  constexpr int NDP = (ND + 3) & ~3;
  __shared__ __attribute__((aligned(16))) float sr[NDP];
  const int lane = threadIdx.x;
  const int64_t cell = xcd_swizzle((int)blockIdx.x, n_cells);
  for (int i = lane; i < NDP; i += 64) sr[i] = i < ND ? (float)r[cell_dofs[cell * ND + i]] : 0.f;
  wave_sync();
  const float *Ac = Ainv + cell * (int64_t)ND * ldi;
  const float4 *r4 = reinterpret_cast<const float4 *>(sr);
  for (int i = lane; i < ND; i += 64) {
    const float4 *row = reinterpret_cast<const float4 *>(Ac + (int64_t)i * ldi);
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < NDP / 4; ++j) {
      const float4 a = row[j], x = r4[j];
      acc += a.x * x.x;
      acc += a.y * x.y;
      acc += a.z * x.z;
      acc += a.w * x.w;
    }
    ev[cell * ND + i] = (double)acc;
  }
}

// x += omega / multiplicity * (sum of the DoF's element-vector slots, ascending cell order)
__global__ void __launch_bounds__(256) k_vanka_update(double *__restrict__ x, const double *__restrict__ ev,
                                                      const int64_t *__restrict__ voff, const int64_t *__restrict__ vslot,
                                                      int64_t nv, const int64_t *__restrict__ poff,
                                                      const int64_t *__restrict__ pslot, int64_t np, int dim, double omega) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    double acc[3] = {0., 0., 0.};
    const int64_t j0 = voff[i], j1 = voff[i + 1];
    for (int64_t j = j0; j < j1; ++j) {
      const double *e = ev + vslot[j];
      for (int c = 0; c < dim; ++c) acc[c] += e[c];
    }
    if (j1 > j0) {
      const double w = omega / (double)(j1 - j0);
      for (int c = 0; c < dim; ++c) x[i * dim + c] += w * acc[c];
    }
  } else if (i < nv + np) {
    const int64_t q = i - nv, j0 = poff[q], j1 = poff[q + 1];
    double acc = 0.;
    for (int64_t j = j0; j < j1; ++j) acc += ev[pslot[j]];
    if (j1 > j0) x[dim * nv + q] += omega / (double)(j1 - j0) * acc;
  }
}

}  // namespace

int vanka_row_floats(int nd) { return (nd + 3) & ~3; }

hipError_t launch_vanka_element(int kp, const OpParams &P, const Tables1D &T, double *K, hipStream_t s) {
  if (P.n_cells <= 0) return hipSuccess;
  if (!P.cq || (kp != 1 && kp != 2)) return hipErrorNotSupported;
  const dim3 g((unsigned)P.n_cells), b(256);
  if (kp == 1) {
    if (P.gq) hipLaunchKernelGGL((k_vanka_element<1, true>), g, b, 0, s, P, T, K);
    else hipLaunchKernelGGL((k_vanka_element<1, false>), g, b, 0, s, P, T, K);
  } else {
    if (P.gq) hipLaunchKernelGGL((k_vanka_element<2, true>), g, b, 0, s, P, T, K);
    else hipLaunchKernelGGL((k_vanka_element<2, false>), g, b, 0, s, P, T, K);
  }
  return hipGetLastError();
}

hipError_t launch_vanka_patch(int n_cells, int nd, const double *K, const int64_t *nb_off, const int32_t *nb_cell,
                              const int64_t *ov_off, const uint8_t *ov_i, const uint8_t *ov_j, const int32_t *cell_dofs,
                              const uint8_t *con, const double *diag, double *A, hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  if (nd > 255) return hipErrorNotSupported;
  hipLaunchKernelGGL(k_vanka_patch, dim3((unsigned)n_cells), dim3(256), 0, s, nd, K, nb_off, nb_cell, ov_off, ov_i, ov_j,
                     cell_dofs, con, diag, A);
  return hipGetLastError();
}

hipError_t launch_vanka_invert(int n_cells, int nd, const double *A, float *Ainv, int32_t *flag, hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  const int ldi = vanka_row_floats(nd);
  if (nd == 89) hipLaunchKernelGGL((k_vanka_invert<89>), dim3((unsigned)n_cells), dim3(256), 0, s, A, Ainv, ldi, flag);
  else if (nd == 108) hipLaunchKernelGGL((k_vanka_invert<108>), dim3((unsigned)n_cells), dim3(256), 0, s, A, Ainv, ldi, flag);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

hipError_t launch_vanka_apply(int n_cells, int nd, const float *Ainv, const int32_t *cell_dofs, const double *r, double *ev,
                              hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  const int ldi = vanka_row_floats(nd);
  if (nd == 89) hipLaunchKernelGGL((k_vanka_apply<89>), dim3((unsigned)n_cells), dim3(64), 0, s, n_cells, Ainv, ldi, cell_dofs, r, ev);
  else if (nd == 108) hipLaunchKernelGGL((k_vanka_apply<108>), dim3((unsigned)n_cells), dim3(64), 0, s, n_cells, Ainv, ldi, cell_dofs, r, ev);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

hipError_t launch_vanka_update(double *x, const double *ev, const int64_t *voff, const int64_t *vslot, int64_t nv,
                               const int64_t *poff, const int64_t *pslot, int64_t np, int dim, double omega, hipStream_t s) {
  const int64_t n = nv + np;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vanka_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ev, voff, vslot, nv, poff, pslot,
                     np, dim, omega);
  return hipGetLastError();
}

}  // namespace gls
