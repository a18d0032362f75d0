// gls_cell_point.hpp -- the per-cell J.v's pointwise algebra at one quadrature point of a 3D Q2 cell, from the
// linearization cache: shared by the sum-factorized J.v (gls_cell_sf.hip) and the element matrices of the cell-Vanka
// smoother (gls_vanka.hip), which apply it to the unit vectors.
#pragma once
#include "gls_common.hpp"

namespace gls {

// The J.v's pointwise part at quadrature point q = i + 3 j + 9 k of `cell` (gls_navier_stokes.cc:548-622):
// v's value, reference gradient and reference Hessian (xx yy zz xy xz yz) per velocity component, the pressure
// value and reference gradient in; the 16 test coefficients out (velocity c: value and reference-gradient
// coefficients at 4c, pressure at 12), with the MappingQ (GEN) or box geometry and the linearization cache.
template <bool GEN>
__device__ __forceinline__ void jv_point(const OpParams &P, int64_t cell, int q, int i, int j, int k, const double *sW,
                                         double (&v)[3], double (&gv)[3][3], const double (&H)[3][6], double vp,
                                         double (&gvp)[3], double (&tc)[16]) {
  // geometry
  double JI[3][3], JxW, lv[3];
  double ih[3] = {1.0, 1.0, 1.0};
  if constexpr (GEN) {
    const double *g = P.gq + (cell * 27 + q) * kGeo;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int e = 0; e < 3; ++e) JI[a][e] = g[kGeoJI + 3 * a + e];
    double Gm[6], cg[3];
#pragma unroll
    for (int t = 0; t < 6; ++t) Gm[t] = g[kGeoG + t];
#pragma unroll
    for (int t = 0; t < 3; ++t) cg[t] = g[kGeoC + t];
    JxW = g[kGeoJxW];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double L = Gm[0] * H[c][0] + Gm[1] * H[c][1] + 2 * Gm[3] * H[c][3] + Gm[2] * H[c][2] + 2 * Gm[4] * H[c][4] +
                 2 * Gm[5] * H[c][5];
      double o[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) o[e] = JI[0][e] * gv[c][0] + JI[1][e] * gv[c][1] + JI[2][e] * gv[c][2];
#pragma unroll
      for (int e = 0; e < 3; ++e) gv[c][e] = o[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) L -= cg[e] * gv[c][e];
      lv[c] = L;
    }
    double o[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = JI[0][e] * gvp[0] + JI[1][e] * gvp[1] + JI[2][e] * gvp[2];
#pragma unroll
    for (int e = 0; e < 3; ++e) gvp[e] = o[e];
  } else {
    const double hx = P.geo[cell * 4 + 0], hy = P.geo[cell * 4 + 1], hz = P.geo[cell * 4 + 2];
    ih[0] = 1.0 / hx;
    ih[1] = 1.0 / hy;
    ih[2] = 1.0 / hz;
    JxW = sW[i] * sW[j] * sW[k] * hx * hy * hz;
    const double wy = (hx * hx) / (hy * hy), wz = (hx * hx) / (hz * hz), il2 = ih[0] * ih[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lv[c] = (H[c][0] + wy * H[c][1] + wz * H[c][2]) * il2;
#pragma unroll
      for (int e = 0; e < 3; ++e) gv[c][e] *= ih[e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) gvp[e] *= ih[e];
  }
  // the linearization cache of this point (u, grad u, tau, R_s)
  const double *cq = P.cq + cell * 16 * 27 + q;
  double u[3], gu[3][3], R[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) u[c] = cq[c * 27];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 3; ++e) gu[c][e] = cq[(3 + 3 * c + e) * 27];
  const double tau = cq[12 * 27];
#pragma unroll
  for (int c = 0; c < 3; ++c) R[c] = cq[(13 + c) * 27];

  const double nu = P.nu, aj = P.alpha_jac;
  double S[3], A[3], divv = 0.;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double gvu = 0., guv = 0.;
#pragma unroll
    for (int e = 0; e < 3; ++e) { guv += gu[c][e] * v[e]; gvu += gv[c][e] * u[e]; }
    A[c] = guv + gvu + aj * v[c];
    S[c] = guv + gvu + gvp[c] - nu * lv[c] + aj * v[c];
    divv += gv[c][c];
  }
  if (P.srf) {
    const double *om = P.omega;
    const double cj[3] = {2 * (om[1] * v[2] - om[2] * v[1]), 2 * (om[2] * v[0] - om[0] * v[2]),
                          2 * (om[0] * v[1] - om[1] * v[0])};
#pragma unroll
    for (int c = 0; c < 3; ++c) { A[c] += cj[c]; S[c] += cj[c]; }
  }
  auto to_ref = [&](double (&t)[3]) {
    if constexpr (GEN) {
      double o[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) o[a] = JI[a][0] * t[0] + JI[a][1] * t[1] + JI[a][2] * t[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = o[a];
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] *= ih[a];
    }
  };
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    tc[4 * c] = JxW * A[c];
    double t[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = JxW * (nu * gv[c][e] - (c == e ? vp : 0.0) + tau * S[c] * u[e] + tau * R[c] * v[e]);
    to_ref(t);
#pragma unroll
    for (int e = 0; e < 3; ++e) tc[4 * c + 1 + e] = t[e];
  }
  tc[12] = JxW * divv;
  {
    double t[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = JxW * tau * S[e];
    to_ref(t);
#pragma unroll
    for (int e = 0; e < 3; ++e) tc[13 + e] = t[e];
  }
}

}  // namespace gls
