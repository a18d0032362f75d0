// gls_lattice_eval.hpp -- fields of a block's cells on a tensor lattice of reference points, sum-factorized through
// LDS from 1D tables (device code shared by gls_output.hip, whose lattice is the patch points, and gls_error.hip,
// whose lattice is QGauss(k+2)). A field of a cell owns one LDS region: nodal values [n^dim] | A | B, where
//   A: x sweep, (t0, a1, a2) <- sum_a0 {V, D}[t0][a0] f[a0, a1, a2]
//   B: y sweep (3D), (t0, t1, a2) <- sum_a1 of {V A_v, V A_d, D A_v}
// and each lane finishes its own point with the last direction in registers. n: nodes per direction of the field,
// np1: lattice points per direction, V / D: [np1][n] basis values / derivatives at the lattice points. DER: the
// sweeps carry the reference derivatives too. The sweeps' items are dealt to all lanes of the block, whichever
// cell they belong to; the caller separates gather, sweep A, sweep B and finish by __syncthreads().
#pragma once
#include <hip/hip_runtime.h>

namespace gls {

__host__ __device__ constexpr int opow(int n, int e) { return e <= 0 ? 1 : n * opow(n, e - 1); }

// LDS doubles of one field of one cell: nodal values | A | B.  der: the sweeps carry the derivatives too
__host__ __device__ inline int field_items_a(int dim, int n, int np1) { return np1 * opow(n, dim - 1); }
__host__ __device__ inline int field_items_b(int dim, int n, int np1) { return dim == 3 ? np1 * np1 * n : 0; }
__host__ __device__ inline int field_doubles(int dim, int n, int np1, bool der) {
  return opow(n, dim) + (der ? 2 : 1) * field_items_a(dim, n, np1) + (der ? 3 : 1) * field_items_b(dim, n, np1);
}

// x sweep of one field of the block's ncl cells. f: the field's region in cell 0, cs: the cells' stride
template <int DIM, bool DER>
__device__ __forceinline__ void sweep_a(double *f, int cs, int ncl, int n, int np1, const double *V, const double *D) {
  const int nod = opow(n, DIM), ia = field_items_a(DIM, n, np1);
  for (int i = threadIdx.x; i < ncl * ia; i += blockDim.x) {
    const int cl = i / ia, r = i - cl * ia, t0 = r % np1, rest = r / np1;
    const double *src = f + cl * cs + n * rest;
    double v = 0.0, d = 0.0;
    for (int a = 0; a < n; ++a) {
      v += V[t0 * n + a] * src[a];
      if (DER) d += D[t0 * n + a] * src[a];
    }
    double *dst = f + cl * cs + nod;
    dst[r] = v;
    if (DER) dst[ia + r] = d;
  }
}

// y sweep (3D): B_vv | B_dv (x derivative) | B_vd (y derivative)
template <bool DER>
__device__ __forceinline__ void sweep_b(double *f, int cs, int ncl, int n, int np1, const double *V, const double *D) {
  const int nod = n * n * n, ia = np1 * n * n, ib = np1 * np1 * n, wa = DER ? 2 : 1;
  for (int i = threadIdx.x; i < ncl * ib; i += blockDim.x) {
    const int cl = i / ib, r = i - cl * ib, t0 = r % np1, t1 = (r / np1) % np1, a2 = r / (np1 * np1);
    const double *av = f + cl * cs + nod + t0 + np1 * n * a2;
    double vv = 0.0, dv = 0.0, vd = 0.0;
    for (int a = 0; a < n; ++a) {
      const double x = av[np1 * a];
      vv += V[t1 * n + a] * x;
      if (DER) {
        dv += V[t1 * n + a] * av[ia + np1 * a];
        vd += D[t1 * n + a] * x;
      }
    }
    double *dst = f + cl * cs + nod + wa * ia;
    dst[r] = vv;
    if (DER) {
      dst[ib + r] = dv;
      dst[2 * ib + r] = vd;
    }
  }
}

// the last direction at the lane's own point: value and reference gradient of one field of its cell
template <int DIM, bool DER>
__device__ __forceinline__ void finish(const double *f, int n, int np1, const int (&tt)[3], const double *V,
                                       const double *D, double &val, double (&g)[3]) {
  const int nod = opow(n, DIM), ia = field_items_a(DIM, n, np1);
  val = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  if constexpr (DIM == 3) {
    const int ib = np1 * np1 * n;
    const double *b = f + nod + (DER ? 2 : 1) * ia + tt[0] + np1 * tt[1];
    for (int a = 0; a < n; ++a) {
      const double vv = b[np1 * np1 * a], v = V[tt[2] * n + a];
      val += v * vv;
      if (DER) {
        g[0] += v * b[ib + np1 * np1 * a];
        g[1] += v * b[2 * ib + np1 * np1 * a];
        g[2] += D[tt[2] * n + a] * vv;
      }
    }
  } else {
    const double *av = f + nod + tt[0];
    for (int a = 0; a < n; ++a) {
      const double x = av[np1 * a], v = V[tt[1] * n + a];
      val += v * x;
      if (DER) {
        g[0] += v * av[ia + np1 * a];
        g[1] += D[tt[1] * n + a] * x;
      }
    }
  }
}

// ---- the transposed sweeps (gls_mass.hip): the lanes' weighted point values q [np1^dim] (x fastest, one array per
// field and cell, cs apart like the regions) integrated back against the basis, through the same regions in the
// reverse order: q -> B -> A -> nodal sums (3D), q -> A -> nodal sums (2D). Values only; the caller separates the
// steps by __syncthreads().
// last direction: B[t0, t1, a2] = sum_t2 V[t2][a2] q[t0, t1, t2] (3D), A[t0, a1] = sum_t1 V[t1][a1] q[t0, t1] (2D)
template <int DIM>
__device__ __forceinline__ void sweep_t_last(double *f, const double *q, int cs, int ncl, int n, int np1,
                                             const double *V) {
  const int nod = opow(n, DIM), ia = field_items_a(DIM, n, np1), items = DIM == 3 ? np1 * np1 * n : ia;
  const int plane = opow(np1, DIM - 1);  // points per value of the last coordinate
  for (int i = threadIdx.x; i < ncl * items; i += blockDim.x) {
    const int cl = i / items, r = i - cl * items, pt = r % plane, a = r / plane;
    const double *src = q + cl * cs + pt;
    double v = 0.0;
    for (int t = 0; t < np1; ++t) v += V[t * n + a] * src[plane * t];
    f[cl * cs + nod + (DIM == 3 ? ia : 0) + r] = v;
  }
}

// y direction (3D): A[t0, a1, a2] = sum_t1 V[t1][a1] B[t0, t1, a2]
__device__ __forceinline__ void sweep_t_b(double *f, int cs, int ncl, int n, int np1, const double *V) {
  const int nod = n * n * n, ia = np1 * n * n;
  for (int i = threadIdx.x; i < ncl * ia; i += blockDim.x) {
    const int cl = i / ia, r = i - cl * ia, t0 = r % np1, a1 = (r / np1) % n, a2 = r / (np1 * n);
    const double *b = f + cl * cs + nod + ia + t0 + np1 * np1 * a2;
    double v = 0.0;
    for (int t = 0; t < np1; ++t) v += V[t * n + a1] * b[np1 * t];
    f[cl * cs + nod + r] = v;
  }
}

// x direction: nodal[a0, rest] = sum_t0 V[t0][a0] A[t0, rest]
template <int DIM>
__device__ __forceinline__ void sweep_t_a(double *f, int cs, int ncl, int n, int np1, const double *V) {
  const int nod = opow(n, DIM);
  for (int i = threadIdx.x; i < ncl * nod; i += blockDim.x) {
    const int cl = i / nod, r = i - cl * nod, a0 = r % n, rest = r / n;
    const double *a = f + cl * cs + nod + np1 * rest;
    double v = 0.0;
    for (int t = 0; t < np1; ++t) v += V[t * n + a0] * a[t];
    f[cl * cs + r] = v;
  }
}

}  // namespace gls
