// gls_api.cpp — C-ABI implementation: context lifecycle, operator dispatch, GMRES / BiCGStab, Newton,
// hyper_cube mesh and time-integration coefficients; the last-error string. Host C++17 over HIP. The context struct
// and the helpers shared with the other host files: gls_ctx.hpp; the multigrid: gls_mg.cpp (its coarsest-level
// direct solve: gls_mg_coarse.cpp); the assembled ILU: gls_ilu.cpp (its host-only plan: gls_ilu_plan.cpp); Kelly,
// boundary loads, flow diagnostics and device output: gls_postproc.cpp; the RCCL transport: gls_rccl.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <array>
#include <memory>
#include <string>
#include <vector>
#include <set>

#include "gls_box_mesh.hpp"
#include "gls_ctx.hpp"
#include "gls_incidence.hpp"

using namespace gls_impl;

namespace {

thread_local std::string g_err;

}  // namespace

namespace gls_impl {  // declared in gls_ctx.hpp
int set_err(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace gls_impl

namespace {

// ---------------- time coefficients (host) ----------------
// Variable-step BDF via divided differences of the backward time levels
// (restates source/core/bdf.cc:23-75: alpha = sum_j prod_{i<j}(t0-ti) * delta_j).
void bdf_delta(int p, int n, int j, const double *times, double *out) {
  if (j == 0) {
    for (int i = 0; i <= p; ++i) out[i] = 0.;
    out[n] = 1.;
    return;
  }
  double a[8], b[8];
  bdf_delta(p, n, j - 1, times, a);
  bdf_delta(p, n + 1, j - 1, times, b);
  const double inv = 1.0 / (times[n] - times[n + j]);
  for (int i = 0; i <= p; ++i) out[i] = (a[i] - b[i]) * inv;
}

bool is_sdirk(int s) { return s >= GLS_SDIRK2 && s <= GLS_SDIRK3_3; }

}  // namespace

int gls_internal_set_err(int code, const char *msg) { return set_err(code, "%s", msg); }
int gls_io_set_error(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return set_err(code, "%s", buf);
}

extern "C" {

const char *gls_last_error(void) { return g_err.c_str(); }
const char *gls_version(void) { return "softx_2020_200_amd 0.1 (gfx950)"; }

int gls_bdf_coefficients(int order, const double *dt, int n_dt, double *alpha) {
  if (order < 1 || order > 5 || !dt || !alpha || n_dt < order) return set_err(GLS_EINVAL, "bdf order/dt");
  double times[8];
  for (int i = 0; i <= order; ++i) {
    times[i] = 0.;
    for (int j = 0; j < i; ++j) times[i] -= dt[j];
  }
  for (int i = 0; i <= order; ++i) alpha[i] = 0.;
  double d[8];
  for (int j = 1; j <= order; ++j) {
    double factor = 1.;
    for (int i = 1; i < j; ++i) factor *= times[0] - times[i];
    bdf_delta(order, 0, j, times, d);
    for (int i = 0; i <= order; ++i) alpha[i] += factor * d[i];
  }
  return GLS_OK;
}

// SDIRK2 (alpha = 1 - 1/sqrt(2)) and the 3-stage L-stable SDIRK3 tables of source/core/sdirk.cc:11-44,
// expressed as stage residual coefficients [stage][outcome, step n, intermediate stages...].
int gls_sdirk_coefficients(int order, double dt, double *c) {
  if (!c || dt == 0.) return set_err(GLS_EINVAL, "sdirk args");
  const double sdt = 1. / dt;
  if (order == 2) {
    const double a = (2. - std::sqrt(2.)) / 2.;
    const double v[6] = {1. / a * sdt, -1. / a * sdt, 0., 1. / a * sdt, -(2 * a - 1) / a / a * sdt,
                         -(1 - a) / a / a * sdt};
    std::memcpy(c, v, sizeof(v));
    return GLS_OK;
  }
  if (order == 3) {
    const double g = 2.29428036027904;
    const double v[12] = {g, -g, 0., 0., g, -0.809559354637498, -1.48472100564154, 0.,
                          g, 2.87009860433106, -8.55612780155264, 3.39174883694255};
    for (int i = 0; i < 12; ++i) c[i] = v[i] * sdt;
    return GLS_OK;
  }
  return set_err(GLS_EINVAL, "sdirk order %d", order);
}

}  // extern "C"

// ============================================================================================
// FE tables
// ============================================================================================
namespace {

void legendre_pd(int n, double x, double &P, double &dP) {
  double p0 = 1., p1 = x;
  if (n == 0) { P = 1.; dP = 0.; return; }
  for (int m = 2; m <= n; ++m) {
    const double p2 = ((2. * m - 1.) * x * p1 - (m - 1.) * p0) / m;
    p0 = p1;
    p1 = p2;
  }
  P = p1;
  dP = n * (x * p1 - p0) / (x * x - 1.);
}

}  // namespace
namespace gls_impl {  // declared in gls_ctx.hpp
// QGauss(n) on [0,1]: Newton on the Legendre roots, ascending.
void gauss_points(int n, double *x, double *w) {
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), P, dP;
    for (int it = 0; it < 100; ++it) {
      legendre_pd(n, z, P, dP);
      const double dz = P / dP;
      z -= dz;
      if (std::fabs(dz) < 1e-17) break;
    }
    legendre_pd(n, z, P, dP);
    x[n - 1 - i] = 0.5 * (1. + z);
    w[n - 1 - i] = 1. / ((1. - z * z) * dP * dP);
  }
}

// FE_Q support points (Gauss–Lobatto) on [0,1]
void lobatto_points(int k, double *x) {
  x[0] = 0.;
  x[k] = 1.;
  for (int i = 1; i < k; ++i) {
    double z = -std::cos(M_PI * i / k);
    for (int it = 0; it < 100; ++it) {
      double P, dP;
      legendre_pd(k, z, P, dP);
      const double d2P = (2. * z * dP - k * (k + 1.) * P) / (1. - z * z);
      const double dz = dP / d2P;
      z -= dz;
      if (std::fabs(dz) < 1e-17) break;
    }
    x[i] = 0.5 * (1. + z);
  }
  if (k == 2) x[1] = 0.5;
}

// Lagrange basis i on nodes xn (degree k): value, first and second derivative at s,
// via the barycentric-style product expansions.
void lagrange_1d(int k, const double *xn, int i, double s, double &v, double &d, double &dd) {
  v = 1.;
  d = 0.;
  dd = 0.;
  for (int j = 0; j <= k; ++j)
    if (j != i) v *= (s - xn[j]) / (xn[i] - xn[j]);
  for (int m = 0; m <= k; ++m) {
    if (m == i) continue;
    double t = 1. / (xn[i] - xn[m]);
    for (int j = 0; j <= k; ++j)
      if (j != i && j != m) t *= (s - xn[j]) / (xn[i] - xn[j]);
    d += t;
    for (int l = 0; l <= k; ++l) {
      if (l == i || l == m) continue;
      double t2 = 1. / ((xn[i] - xn[m]) * (xn[i] - xn[l]));
      for (int j = 0; j <= k; ++j)
        if (j != i && j != m && j != l) t2 *= (s - xn[j]) / (xn[i] - xn[j]);
      dd += t2;
    }
  }
}
}  // namespace gls_impl
namespace {

gls::Tables1D make_tables(int k, int kp, int nq1d) {
  gls::Tables1D T;
  std::memset(&T, 0, sizeof(T));
  double xq[gls::kMaxQ1D], wq[gls::kMaxQ1D], xv[gls::kMaxNodes1D], xp[gls::kMaxNodes1D];
  gauss_points(nq1d, xq, wq);
  lobatto_points(k, xv);
  lobatto_points(kp, xp);
  for (int q = 0; q < nq1d; ++q) {
    T.w[q] = wq[q];
    T.xi[q] = xq[q];
    for (int a = 0; a <= k; ++a) lagrange_1d(k, xv, a, xq[q], T.V[q][a], T.D[q][a], T.S[q][a]);
    for (int a = 0; a <= kp; ++a) {
      double dd;
      lagrange_1d(kp, xp, a, xq[q], T.Vp[q][a], T.Dp[q][a], dd);
    }
  }
  return T;
}

}  // namespace

namespace {

// The brick kernels need: 3D, equal order k==kp in {1,2}, QGauss(k+1), pressure on the velocity
// nodes, and every 8 consecutive cells forming a conforming 2x2x2 brick (Morton order) whose
// interior nodes belong to no other brick (they are written with plain stores).
bool detect_bricks(const gls_mesh_desc *d, int nq1d) {
  if (getenv("GLS_DISABLE_BRICK")) return false;
  if (d->dim != 3 || d->k != d->kp || (d->k != 1 && d->k != 2) || nq1d != d->k + 1) return false;
  if (d->cell_pnodes || d->n_cells % 8 != 0 || d->n_cells == 0) return false;
  const int K = d->k, K1 = K + 1, N3 = K1 * K1 * K1, BN = 2 * K + 1;
  const int nb = d->n_cells / 8;
  std::vector<int32_t> owner((size_t)d->n_vnodes, -1);
  std::vector<int32_t> bnode((size_t)BN * BN * BN);
  for (int b = 0; b < nb; ++b) {
    std::fill(bnode.begin(), bnode.end(), -1);
    for (int cc = 0; cc < 8; ++cc) {
      const int cx = cc & 1, cy = (cc >> 1) & 1, cz = cc >> 2;
      const int32_t *cv = d->cell_vnodes + ((size_t)b * 8 + cc) * N3;
      for (int a = 0; a < N3; ++a) {
        const int ax = a % K1, ay = (a / K1) % K1, az = a / (K1 * K1);
        const int n = (K * cx + ax) + BN * ((K * cy + ay) + BN * (K * cz + az));
        if (bnode[n] == -1) bnode[n] = cv[a];
        else if (bnode[n] != cv[a]) return false;  // not a conforming brick
      }
    }
    for (int Z = 1; Z < BN - 1; ++Z)
      for (int Y = 1; Y < BN - 1; ++Y)
        for (int X = 1; X < BN - 1; ++X) {
          const int32_t node = bnode[X + BN * (Y + BN * Z)];
          if (owner[node] != -1) return false;
          owner[node] = b;
        }
  }
  for (int cix = 0; cix < d->n_cells; ++cix)
    for (int a = 0; a < N3; ++a) {
      const int32_t o = owner[d->cell_vnodes[(size_t)cix * N3 + a]];
      if (o != -1 && o != cix / 8) return false;
    }
  return true;
}

// node -> slab slots of the bricks whose surface holds it (CSR sorted by node, slots ascending)
int build_slab_map(gls_ctx *c, const gls_mesh_desc *d) {
  const int K = d->k, K1 = K + 1, N3 = K1 * K1 * K1, BN = 2 * K + 1;
  const int nbnd = gls::brick_boundary_nodes(K);
  const int64_t nb = d->n_cells / 8;
  if (nb * nbnd >= INT32_MAX) return GLS_OK;  // keep atomics beyond int32 slot ids
  std::vector<int32_t> cnt((size_t)d->n_vnodes + 1, 0), slot_node((size_t)(nb * nbnd));
  for (int64_t b = 0; b < nb; ++b) {
    int j = 0;
    for (int Z = 0; Z < BN; ++Z)
      for (int Y = 0; Y < BN; ++Y)
        for (int X = 0; X < BN; ++X) {
          if (X > 0 && X < BN - 1 && Y > 0 && Y < BN - 1 && Z > 0 && Z < BN - 1) continue;
          const int cx = std::min(X / K, 1), cy = std::min(Y / K, 1), cz = std::min(Z / K, 1);
          const int a = (X - K * cx) + K1 * ((Y - K * cy) + K1 * (Z - K * cz));
          const int32_t node = d->cell_vnodes[((size_t)b * 8 + cx + 2 * cy + 4 * cz) * N3 + a];
          slot_node[(size_t)(b * nbnd + j)] = node;
          ++cnt[(size_t)node + 1];
          ++j;
        }
    if (j != nbnd) return set_err(GLS_EINVAL, "brick boundary count %d != %d", j, nbnd);
  }
  std::vector<int32_t> nodes, off{0};
  std::vector<int32_t> start((size_t)d->n_vnodes + 1, 0);
  for (int64_t n = 0; n < d->n_vnodes; ++n) {
    start[(size_t)n + 1] = start[(size_t)n] + cnt[(size_t)n + 1];
    if (cnt[(size_t)n + 1] > 0) {
      nodes.push_back((int32_t)n);
      off.push_back(start[(size_t)n + 1]);
    }
  }
  std::vector<int32_t> slots((size_t)(nb * nbnd)), fill(start.begin(), start.end() - 1);
  for (int64_t sl = 0; sl < nb * nbnd; ++sl) slots[(size_t)fill[(size_t)slot_node[(size_t)sl]]++] = (int32_t)sl;
  const std::vector<int32_t> slots_by_node = slots;  // node n's slots at [start[n], start[n+1])
  // sum order: nodes by their first (lowest) slot, i.e. in slab order of their lowest brick, so
  // that consecutive threads of k_slab_sum read consecutive slab entries (node order would leave
  // the x-face nodes of every brick row 4 lattice points apart: 2.3x read amplification, PMC)
  {
    const size_t m = nodes.size();
    std::vector<int32_t> perm(m);
    for (size_t i = 0; i < m; ++i) perm[i] = (int32_t)i;
    std::sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return slots[(size_t)off[a]] < slots[(size_t)off[b]]; });
    std::vector<int32_t> n2(m), off2{0}, s2;
    s2.reserve(slots.size());
    for (size_t i = 0; i < m; ++i) {
      const int32_t a = perm[i];
      n2[i] = nodes[(size_t)a];
      for (int32_t j = off[(size_t)a]; j < off[(size_t)a + 1]; ++j) s2.push_back(slots[(size_t)j]);
      off2.push_back((int32_t)s2.size());
    }
    nodes.swap(n2);
    off.swap(off2);
    slots.swap(s2);
  }
  GLS_TRY(c->sum_nodes.upload(nodes.data(), nodes.size()));
  GLS_TRY(c->sum_off.upload(off.data(), off.size()));
  GLS_TRY(c->sum_slots.upload(slots.data(), slots.size()));
  c->use_slab = true;
  // structured hyper_cube (gls_mesh_hyper_cube: lexicographic node lattice, cells in Morton order, no
  // periodic wrap): verified cell by cell, then the slab sums run without the index arrays
  c->cube_nb1 = 0;
  if (!std::getenv("GLS_SLAB_CSR")) {
    int64_t n = (int64_t)std::llround(std::cbrt((double)d->n_cells));
    const int64_t NX = K * n + 1;
    bool ok = n >= 2 && n % 2 == 0 && n * n * n == d->n_cells && NX * NX * NX == d->n_vnodes && n <= 2048;
    for (int64_t cl = 0; ok && cl < d->n_cells; ++cl) {
      const int64_t b = cl / 8, ci = cl % 8;
      int64_t bx = 0, by = 0, bz = 0;
      for (int bit = 0; bit < 21; ++bit) {
        bx |= ((b >> (3 * bit)) & 1) << bit;
        by |= ((b >> (3 * bit + 1)) & 1) << bit;
        bz |= ((b >> (3 * bit + 2)) & 1) << bit;
      }
      if (bx >= n / 2 || by >= n / 2 || bz >= n / 2) { ok = false; break; }
      const int64_t x0 = K * (2 * bx + (ci & 1)), y0 = K * (2 * by + ((ci >> 1) & 1)), z0 = K * (2 * bz + (ci >> 2));
      for (int a = 0; a < N3 && ok; ++a) {
        const int ax = a % K1, ay = (a / K1) % K1, az = a / (K1 * K1);
        ok = d->cell_vnodes[(size_t)cl * N3 + a] == (int32_t)((x0 + ax) + NX * ((y0 + ay) + NX * (z0 + az)));
      }
    }
    if (ok) c->cube_nb1 = (int)(n / 2);
  }
  // open subdivided hyper_rectangle (gls_mesh_hyper_rectangle, mask 0: lexicographic node lattice, bricks in
  // tile-Morton order), verified cell by cell like the cube; consulted only where cube_nb1 == 0
  c->box_nb[0] = c->box_nb[1] = c->box_nb[2] = 0;
  c->box_s = 0;
  if (!std::getenv("GLS_SLAB_CSR")) {
    int nbb[3], s = 0;
    if (gls_impl::box_lattice_detect(d->n_cells, d->n_vnodes, K, d->cell_vnodes, nbb, &s)) {
      for (int a = 0; a < 3; ++a) c->box_nb[a] = nbb[a];
      c->box_s = s;
    }
  }
  // brick coloring: greedy in brick (Morton) order over the bricks sharing a surface node
  if (!gls::brick_colors_supported(K)) return GLS_OK;  // only in a -DGLS_BRICK_COLORS_BUILD library (A/B)
  std::vector<int> color((size_t)nb, -1);
  int ncol = 0;
  for (int64_t b = 0; b < nb; ++b) {
    uint32_t used = 0;
    for (int j = 0; j < nbnd; ++j) {
      const int32_t node = slot_node[(size_t)(b * nbnd + j)];
      for (int32_t t = start[(size_t)node]; t < start[(size_t)node + 1]; ++t) {
        const int64_t ob = slots_by_node[(size_t)t] / nbnd;
        if (ob != b && color[(size_t)ob] >= 0) used |= 1u << color[(size_t)ob];
      }
    }
    int col = 0;
    while (col < 32 && ((used >> col) & 1u)) ++col;
    if (col >= 16) return GLS_OK;  // more than 16 colors: keep the slab path
    color[(size_t)b] = col;
    ncol = std::max(ncol, col + 1);
  }
  std::vector<uint16_t> ncm((size_t)d->n_vnodes, 0);
  for (int64_t sl = 0; sl < nb * nbnd; ++sl) ncm[(size_t)slot_node[(size_t)sl]] |= (uint16_t)(1u << color[(size_t)(sl / nbnd)]);
  std::vector<int32_t> order;
  order.reserve((size_t)nb);
  c->color_off[0] = 0;
  for (int col = 0; col < ncol; ++col) {
    for (int64_t b = 0; b < nb; ++b)
      if (color[(size_t)b] == col) order.push_back((int32_t)b);
    c->color_off[col + 1] = (int)order.size();
  }
  GLS_TRY(c->color_bricks.upload(order.data(), order.size()));
  GLS_TRY(c->ncolor.upload(ncm.data(), ncm.size()));
  c->n_colors = ncol;
  c->use_colors = true;
  return GLS_OK;
}

// colored brick launch: surface-node sums carried in acc (y, or scratch for the fused Jacobi sweep)
void set_colors(gls_ctx *c, gls::OpParams &P, double *acc) {
  P.bricks = c->color_bricks.p;
  P.ncolor = c->ncolor.p;
  P.acc = acc;
  P.n_colors = c->n_colors;
  for (int i = 0; i <= c->n_colors; ++i) P.color_off[i] = c->color_off[i];
  P.slab = nullptr;
  P.slabf = nullptr;
}

// MappingQ(md) on one cell at the QGauss(nq1d) points: x_q, JxW, J^-1, G = J^-1 J^-T and the
// Hessian correction c_k = sum_ab G_ab d2x_k/dxi_a dxi_b (kGeo layout, gls_common.hpp); support
// points S[(md+1)^dim][dim] on the equidistant lattice (Gauss-Lobatto for md <= 2)
void mapped_geometry(int dim, int md, int nq1d, const double *S, double *out) {
  double xq[gls::kMaxQ1D], wq[gls::kMaxQ1D];
  gauss_points(nq1d, xq, wq);
  const int m1 = md + 1, ns = gls::ipow(m1, dim), nq = gls::ipow(nq1d, dim);
  double xn[4];
  for (int i = 0; i <= md; ++i) xn[i] = (double)i / md;
  double L[gls::kMaxQ1D][4], dL[gls::kMaxQ1D][4], ddL[gls::kMaxQ1D][4];
  for (int q = 0; q < nq1d; ++q)
    for (int a = 0; a <= md; ++a) lagrange_1d(md, xn, a, xq[q], L[q][a], dL[q][a], ddL[q][a]);
  for (int q = 0; q < nq; ++q) {
    const int qi[3] = {q % nq1d, (q / nq1d) % nq1d, dim == 3 ? q / (nq1d * nq1d) : 0};
    double x[3] = {0, 0, 0}, J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    double H[3][3][3] = {};
    for (int b = 0; b < ns; ++b) {
      const int ib[3] = {b % m1, (b / m1) % m1, dim == 3 ? b / (m1 * m1) : 0};
      double v[3], dv[3], ddv[3];
      for (int d = 0; d < 3; ++d) {
        v[d] = d < dim ? L[qi[d]][ib[d]] : 1.0;
        dv[d] = d < dim ? dL[qi[d]][ib[d]] : 0.0;
        ddv[d] = d < dim ? ddL[qi[d]][ib[d]] : 0.0;
      }
      const double N = v[0] * v[1] * v[2];
      double g[3], h[3][3];
      for (int a = 0; a < dim; ++a) {
        g[a] = 1.0;
        for (int d = 0; d < dim; ++d) g[a] *= d == a ? dv[d] : v[d];
        for (int a2 = 0; a2 < dim; ++a2) {
          h[a][a2] = 1.0;
          for (int d = 0; d < dim; ++d) h[a][a2] *= (d == a && d == a2) ? ddv[d] : ((d == a || d == a2) ? dv[d] : v[d]);
        }
      }
      for (int i = 0; i < dim; ++i) {
        const double Sb = S[b * dim + i];
        x[i] += N * Sb;
        for (int a = 0; a < dim; ++a) {
          J[i][a] += Sb * g[a];
          for (int a2 = 0; a2 < dim; ++a2) H[i][a][a2] += Sb * h[a][a2];
        }
      }
    }
    double det, JI[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (dim == 2) {
      det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      JI[0][0] = J[1][1] / det;
      JI[0][1] = -J[0][1] / det;
      JI[1][0] = -J[1][0] / det;
      JI[1][1] = J[0][0] / det;
    } else {
      det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
            J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      for (int a = 0; a < 3; ++a)
        for (int i = 0; i < 3; ++i) {  // inverse = adjugate / det: JI[a][i] = cof(J)[i][a] / det
          const int r0 = (i + 1) % 3, r1 = (i + 2) % 3, c0 = (a + 1) % 3, c1 = (a + 2) % 3;
          JI[a][i] = (J[r0][c0] * J[r1][c1] - J[r0][c1] * J[r1][c0]) / det;
        }
    }
    double G[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < dim; ++a)
      for (int b = 0; b < dim; ++b)
        for (int i = 0; i < dim; ++i) G[a][b] += JI[a][i] * JI[b][i];
    double *o = out + (size_t)q * gls::kGeo;
    for (int i = 0; i < gls::kGeo; ++i) o[i] = 0.0;
    double w = 1.0;
    for (int d = 0; d < dim; ++d) w *= wq[qi[d]];
    for (int i = 0; i < dim; ++i) o[gls::kGeoX + i] = x[i];
    o[gls::kGeoJxW] = w * det;
    for (int a = 0; a < dim; ++a)
      for (int i = 0; i < dim; ++i) o[gls::kGeoJI + 3 * a + i] = JI[a][i];
    o[gls::kGeoG + 0] = G[0][0];
    o[gls::kGeoG + 1] = G[1][1];
    o[gls::kGeoG + 2] = G[2][2];
    o[gls::kGeoG + 3] = G[0][1];
    o[gls::kGeoG + 4] = G[0][2];
    o[gls::kGeoG + 5] = G[1][2];
    for (int k = 0; k < dim; ++k) {
      double cs = 0;
      for (int a = 0; a < dim; ++a)
        for (int b = 0; b < dim; ++b) cs += G[a][b] * H[k][a][b];
      o[gls::kGeoC + k] = cs;
    }
  }
}

}  // namespace
namespace gls_impl {  // declared in gls_ctx.hpp
// brick launch output: slab (allocated on first use) or nullptr (atomics into a zeroed y)
double *brick_slab(gls_ctx *c) {
  if (!c->use_slab) return nullptr;
  const size_t n = (size_t)(c->n_cells / 8) * gls::brick_boundary_nodes(c->k) * 4;
  if (c->slab.n != n && c->slab.alloc(n) != GLS_OK) return nullptr;
  return c->slab.p;
}

// cell->measure() of a mapped cell from its corner support points (exact bilinear / trilinear
// volume: 2-point Gauss of the multilinear det J)
double corner_measure(int dim, int md, const double *S) {
  const int m1 = md + 1;
  double X[8][3] = {};
  for (int v = 0; v < (1 << dim); ++v) {
    const int b = (v & 1) * md + m1 * (((v >> 1) & 1) * md + (dim == 3 ? m1 * (((v >> 2) & 1) * md) : 0));
    for (int i = 0; i < dim; ++i) X[v][i] = S[b * dim + i];
  }
  const double g = 0.5 / std::sqrt(3.0), xs[2] = {0.5 - g, 0.5 + g};
  double vol = 0;
  for (int q = 0; q < (1 << dim); ++q) {
    const double xi[3] = {xs[q & 1], xs[(q >> 1) & 1], xs[(q >> 2) & 1]};
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int v = 0; v < (1 << dim); ++v)
      for (int a = 0; a < dim; ++a) {
        double gr = ((v >> a) & 1) ? 1.0 : -1.0;
        for (int b = 0; b < dim; ++b)
          if (b != a) gr *= ((v >> b) & 1) ? xi[b] : 1 - xi[b];
        for (int i = 0; i < dim; ++i) J[i][a] += gr * X[v][i];
      }
    vol += (dim == 2 ? J[0][0] * J[1][1] - J[0][1] * J[1][0]
                     : J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])) /
           (1 << dim);
  }
  return vol;
}

// jac: parameters of the Jacobian operators (the frozen snapshot when gls_freeze_jacobian is on)
gls::OpParams make_params(gls_ctx *c, bool jac) {
  gls::OpParams P;
  std::memset(&P, 0, sizeof(P));
  P.n_cells = c->n_cells;
  P.n_vnodes = c->n_vnodes;
  P.n_pnodes = c->n_pnodes;
  P.n_hist = c->n_hist;
  P.cell_vnodes = c->cell_vnodes.p;
  P.cell_pnodes = c->cell_pnodes.p;
  P.geo = c->geo.p;
  P.x0 = c->x0.p;
  P.gq = c->gq.p;
  P.force_q = c->force_q.p;
  P.vmask = c->vmask.p;
  P.cube_nb1 = c->k == 2 ? c->cube_nb1 : 0;  // the pencil kernels' lattice gather (OpParams::cube_gather)
  P.u = c->u;
  P.h1 = c->u1 ? c->u1 : c->u;
  P.h2 = c->u2 ? c->u2 : c->u;
  P.h3 = c->u3 ? c->u3 : c->u;
  P.nu = c->viscosity;
  for (int i = 0; i < 4; ++i) P.alpha[i] = c->alpha[i];
  P.alpha_jac = c->alpha_jac;
  P.sdt2 = c->sdt2;
  P.srf = c->srf;
  for (int i = 0; i < 3; ++i) P.omega[i] = c->omega[i];
  if (jac && c->jf.on) {
    const auto &j = c->jf;
    P.u = j.u.p;
    P.h1 = j.has[0] ? j.h[0].p : j.u.p;
    P.h2 = j.has[1] ? j.h[1].p : j.u.p;
    P.h3 = j.has[2] ? j.h[2].p : j.u.p;
    P.n_hist = j.n_hist;
    for (int i = 0; i < 4; ++i) P.alpha[i] = j.alpha[i];
    P.alpha_jac = j.alpha_jac;
    P.sdt2 = j.sdt2;
  }
  return P;
}
// ---- distributed hooks (no-ops on a single rank)
int dist_import(gls_ctx *c, double *x) {
  if (!c->dist.on) return GLS_OK;
  if (c->dist.dofs) {
    HIP_TRY(gls::vec_pack_dofs(x, c->dist.send_nodes.p, c->dist.n_send, c->dist.send_buf, c->stream));
    if (c->dist.xchg(c->dist.user, 0) != 0) return set_err(GLS_ECOMM, "ghost import exchange failed");
    HIP_TRY(gls::vec_unpack_dofs(x, c->dist.recv_nodes.p, c->dist.n_recv, c->dist.recv_buf, c->stream));
    return GLS_OK;
  }
  const int64_t voff = 3 * (int64_t)c->n_vnodes;
  HIP_TRY(gls::vec_pack_nodes(x, c->dist.send_nodes.p, c->dist.n_send, voff, c->dist.send_buf, c->stream));
  if (c->dist.xchg(c->dist.user, 0) != 0) return set_err(GLS_ECOMM, "ghost import exchange failed");
  HIP_TRY(gls::vec_unpack_nodes(x, c->dist.recv_nodes.p, c->dist.n_recv, voff, c->dist.recv_buf, 0, c->stream));
  return GLS_OK;
}
int dist_export_add(gls_ctx *c, double *y) {
  if (!c->dist.on) return GLS_OK;
  if (c->dist.dofs) {
    HIP_TRY(gls::vec_pack_dofs(y, c->dist.recv_nodes.p, c->dist.n_recv, c->dist.recv_buf, c->stream));
    if (c->dist.xchg(c->dist.user, 1) != 0) return set_err(GLS_ECOMM, "ghost export exchange failed");
    HIP_TRY(gls::vec_add_dofs_ordered(y, c->dist.add_u.p, c->dist.add_off.p, c->dist.add_slot.p, (int64_t)c->dist.add_u.n,
                                      c->dist.send_buf, c->stream));
    return GLS_OK;
  }
  const int64_t voff = 3 * (int64_t)c->n_vnodes;
  HIP_TRY(gls::vec_pack_nodes(y, c->dist.recv_nodes.p, c->dist.n_recv, voff, c->dist.recv_buf, c->stream));
  if (c->dist.xchg(c->dist.user, 1) != 0) return set_err(GLS_ECOMM, "ghost export exchange failed");
  HIP_TRY(gls::vec_add_nodes_ordered(y, c->dist.add_u.p, c->dist.add_off.p, c->dist.add_slot.p, (int64_t)c->dist.add_u.n,
                                     voff, c->dist.send_buf, c->stream));
  return GLS_OK;
}
// in-place sum over ranks of a device vector through c's transport (RCCL: one call; callback transports
// through their reduction buffer in chunks of GLS_RED_BUF_MIN values)
int dist_allreduce_vector(gls_ctx *c, double *v, int64_t n) {
  auto &D = c->dist;
  if (!D.on) return GLS_OK;
  if (D.comm) {
    if (D.allreduce(D.user, v, (int)n) != 0) return set_err(GLS_ECOMM, "vector all-reduce failed");
    return GLS_OK;
  }
  hipStream_t s = c->stream;
  for (int64_t o = 0; o < n; o += GLS_RED_BUF_MIN) {
    const int len = (int)std::min<int64_t>(GLS_RED_BUF_MIN, n - o);
    HIP_TRY(hipMemcpyAsync(D.red_buf, v + o, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
    if (D.allreduce(D.user, D.red_buf, len) != 0) return set_err(GLS_ECOMM, "vector all-reduce failed");
    HIP_TRY(hipMemcpyAsync(v + o, D.red_buf, sizeof(double) * len, hipMemcpyDeviceToDevice, s));
  }
  return GLS_OK;
}
}  // namespace gls_impl
namespace {

// export-add order: every owned entry's incoming exchange slots in ascending slot (= neighbour) order,
// so the sums over several neighbours are deterministic
int upload_export_order(gls_ctx::Dist &D, const int32_t *send, int64_t ns) {
  std::vector<std::pair<int32_t, int32_t>> ds;
  ds.reserve((size_t)ns);
  for (int64_t j = 0; j < ns; ++j) ds.push_back({send[j], (int32_t)j});
  std::stable_sort(ds.begin(), ds.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) {
    return a.first < b.first;
  });
  std::vector<int32_t> au, aoff{0}, aslot;
  for (size_t t = 0; t < ds.size(); ++t) {
    if (t == 0 || ds[t].first != ds[t - 1].first) {
      if (t) aoff.push_back((int32_t)aslot.size());
      au.push_back(ds[t].first);
    }
    aslot.push_back(ds[t].second);
  }
  if (!au.empty()) aoff.push_back((int32_t)aslot.size());
  GLS_TRY(D.add_u.upload(au.data(), au.size()));
  GLS_TRY(D.add_off.upload(aoff.data(), au.empty() ? 0 : aoff.size()));
  return D.add_slot.upload(aslot.data(), aslot.size());
}
// out[k] = sum over OWNED DoFs of A[k] . w, reduced over ranks (host result)
int dist_multidot(gls_ctx *c, const double *A, int64_t lda, int nk, const double *w, double *host_out) {
  const int64_t n1 = c->dist.on ? (int64_t)c->dim * c->dist.n_owned : c->n_dofs;
  const int64_t off2 = c->dist.on ? (int64_t)c->dim * c->n_vnodes : 0;
  const int64_t n2 = c->dist.on ? c->dist.n_owned_p : 0;
  HIP_TRY(gls::vec_multidot2(A, lda, nk, w, n1, off2, n2, c->scal.p, c->work.p, c->stream));
  if (c->dist.on) {
    HIP_TRY(hipMemcpyAsync(c->dist.red_buf, c->scal.p, sizeof(double) * nk, hipMemcpyDeviceToDevice, c->stream));
    if (c->dist.allreduce(c->dist.user, c->dist.red_buf, nk) != 0) return set_err(GLS_ECOMM, "allreduce failed");
    HIP_TRY(hipMemcpyAsync(host_out, c->dist.red_buf, sizeof(double) * nk, hipMemcpyDeviceToHost, c->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(host_out, c->scal.p, sizeof(double) * nk, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

// a mixed-precision smoothing level gets the FP32 copy of its linearization from the same MODE_LIN
// launch (workgroup brick kernel): no separate FP64 -> FP32 conversion pass over the linearization
int lin_f32_target(gls_ctx *c, gls::OpParams &P) {
  P.qdf = nullptr;
  if (!c->smooth_f32 || !gls::brick_fused_jacobi_supported(c->k)) return GLS_OK;
  if (c->qdata32.n != c->qdata.n) GLS_TRY(c->qdata32.alloc(c->qdata.n));
  P.qdf = c->qdata32.p;
  P.oseen = c->smooth_oseen ? 1 : 0;  // the Oseen smoother reads u and tau only: the other FP32 rows are not written
  return GLS_OK;
}

// the slab node sums with an FP32 slab and / or the fused damped-Jacobi sweep / residual form
hipError_t slab_sum_ex(gls_ctx *g, const double *slab, const float *slabf, double *y, const uint8_t *vmask,
                       const double *jb, const double *jd, double omega, const double *rb, double *x0 = nullptr,
                       const double *xs = nullptr) {
  if (g->cube_nb1 > 0)
    return gls::brick_slab_sum_cube(g->k, g->cube_nb1, slab, slabf, g->n_vnodes, y, vmask, jb, jd, omega, g->stream, rb,
                                    x0, xs);
  if (g->box_nb[0] > 0 && !xs)
    return gls::brick_slab_sum_box(g->k, g->box_nb, g->box_s, slab, slabf, g->n_vnodes, y, vmask, jb, jd, omega, g->stream,
                                   rb, x0);
  if (x0 || xs) return hipErrorInvalidValue;
  return gls::brick_slab_sum_ex(slab, slabf, g->sum_nodes.p, g->sum_off.p, g->sum_slots.p, (int64_t)g->sum_nodes.n,
                                g->n_vnodes, y, vmask, jb, jd, omega, g->stream, rb);
}
hipError_t slab_sum(gls_ctx *c, double *y) {
  if (c->cube_nb1 > 0)
    return gls::brick_slab_sum_cube(c->k, c->cube_nb1, c->slab.p, nullptr, c->n_vnodes, y, nullptr, nullptr, nullptr, 0.0,
                                    c->stream);
  if (c->box_nb[0] > 0)
    return gls::brick_slab_sum_box(c->k, c->box_nb, c->box_s, c->slab.p, nullptr, c->n_vnodes, y, nullptr, nullptr, nullptr,
                                   0.0, c->stream);
  return gls::brick_slab_sum(c->slab.p, c->sum_nodes.p, c->sum_off.p, c->sum_slots.p, (int64_t)c->sum_nodes.n,
                             c->n_vnodes, y, c->stream);
}


// the brick split: a brick is a boundary brick when one of its cells holds a flagged node (ghost or
// exported); boundary bricks first, then interior ones, each in ascending (Morton) order
int build_brick_split(gls_ctx *c, const std::vector<char> &flag) {
  const int nvc = gls::ipow(c->k + 1, 3), nb = c->n_cells / 8;
  std::vector<int32_t> cv((size_t)c->n_cells * nvc);
  HIP_TRY(hipMemcpy(cv.data(), c->cell_vnodes.p, cv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> bnd, inn;
  for (int b = 0; b < nb; ++b) {
    bool on = false;
    for (size_t e = (size_t)b * 8 * nvc; e < (size_t)(b + 1) * 8 * nvc && !on; ++e) on = flag[(size_t)cv[e]] != 0;
    (on ? bnd : inn).push_back(b);
  }
  c->split_bnd = (int)bnd.size();
  c->split_int = (int)inn.size();
  bnd.insert(bnd.end(), inn.begin(), inn.end());
  return c->split.upload(bnd.data(), std::max<size_t>(bnd.size(), 1));
}

// J.v launched as two brick subsets (boundary, then interior) with the ghost import between them:
// the RCCL transport imports on the exchange stream while the interior bricks run
// GLS_SPLIT_TEST=m on a single-GPU context splits at "bricks b % m == 0"
// with no exchange, for the bitwise test of the split launch; GLS_SPLIT_DIST=1 runs the same split
// launch with the callback transport (import first, then interior and boundary bricks), so the
// boundary / interior classification of a real partition is tested without an RCCL communicator
bool split_jv_enabled(gls_ctx *c) {
  if (!c->use_brick || !c->use_qdata || c->use_colors || c->hang.on || !gls::brick_subset_supported(c->k)) return false;
  if (c->dist.on)
    return c->split.p && (c->dist.comm != nullptr || std::getenv("GLS_SPLIT_DIST"));
  const char *t = std::getenv("GLS_SPLIT_TEST");
  if (!t || std::atoi(t) < 1) return false;
  if (!c->split.p) {
    const int m = std::atoi(t), nb = c->n_cells / 8;
    std::vector<int32_t> bnd, inn;
    for (int b = 0; b < nb; ++b) (b % m == 0 ? bnd : inn).push_back(b);
    c->split_bnd = (int)bnd.size();
    c->split_int = (int)inn.size();
    bnd.insert(bnd.end(), inn.begin(), inn.end());
    if (c->split.upload(bnd.data(), std::max<size_t>(bnd.size(), 1)) != GLS_OK) return false;
  }
  return true;
}

}  // namespace
namespace gls_impl {  // declared in gls_ctx.hpp
// J.v linearization (u, grad u, tau, R_s at every quadrature point), once per state
int ensure_qdata(gls_ctx *c) {
  if (c->qd_valid) return GLS_OK;
  const size_t n = gls::brick_qdata_size(c->k, c->n_cells);
  if (c->qdata.n != n) GLS_TRY(c->qdata.alloc(n));
  gls::OpParams P = make_params(c, true);
  P.qd = c->qdata.p;
  GLS_TRY(lin_f32_target(c, P));
  {
    TimedLaunch t(c, 3);
    HIP_TRY(gls::launch_brick_kernel(c->k, gls::MODE_LIN, P, c->tables, c->stream));
  }
  c->qd_valid = true;
  c->qd32_valid = P.qdf != nullptr;
  c->qd32_partial = P.qdf != nullptr && P.oseen;
  return GLS_OK;
}

// slots of every node in the per-cell element vectors [n_cells][NV*dim + NP], ascending (cell, local
// node) order: the fixed summation order of gather_element_vectors
int ensure_element_maps(gls_ctx *c) {
  if (c->ev.p || c->n_cells == 0) return GLS_OK;
  const int dim = c->dim, nv = gls::ipow(c->k + 1, dim), np = gls::ipow(c->kp + 1, dim), el = nv * dim + np;
  std::vector<int32_t> cv((size_t)c->n_cells * nv), cp;
  HIP_TRY(hipMemcpy(cv.data(), c->cell_vnodes.p, cv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (c->cell_pnodes.p) {
    cp.resize((size_t)c->n_cells * np);
    HIP_TRY(hipMemcpy(cp.data(), c->cell_pnodes.p, cp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  const std::vector<int32_t> &pn = c->cell_pnodes.p ? cp : cv;
  ElementIncidence I;
  if (!element_incidence(c->n_cells, dim, nv, np, c->n_vnodes, c->n_pnodes, cv.data(), pn.data(), I))
    return set_err(GLS_EINVAL, "element maps: a cell's node id is out of range");
  GLS_TRY(c->ev_voff.upload(I.voff.data(), I.voff.size()));
  GLS_TRY(c->ev_vslot.upload(I.vslot.data(), std::max<size_t>(I.vslot.size(), 1)));
  GLS_TRY(c->ev_poff.upload(I.poff.data(), I.poff.size()));
  GLS_TRY(c->ev_pslot.upload(I.pslot.data(), std::max<size_t>(I.pslot.size(), 1)));
  return c->ev.alloc((size_t)c->n_cells * el);
}
}  // namespace gls_impl
namespace {

// adapted forest bricks: the pencil linearization (no output) at the current state
int oct_lin(gls_ctx *c) {
  gls::OpParams L = make_params(c, true);
  L.qd = c->qdata.p;
  L.subset = c->oct.list.p;
  L.subset_n = c->oct.nb;
  L.brick_cell0 = c->oct.cell0.p;
  HIP_TRY(gls::launch_pencil_ev(gls::MODE_LIN, L, c->tables, c->stream));
  c->qd_valid = true;
  c->qd32_valid = false;
  return GLS_OK;
}
int run_cell(gls_ctx *c, int mode, const double *v, double *y) {
  if (!c->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  if (c->n_hist > 0 && !c->u1) return set_err(GLS_EINVAL, "scheme needs solution_m1");
  if (c->n_hist > 1 && !c->u2) return set_err(GLS_EINVAL, "scheme needs solution_m2");
  if (c->n_hist > 2 && !c->u3) return set_err(GLS_EINVAL, "scheme needs solution_m3");
  // per-cell J.v from the diagonal pass's linearization cache
  const bool cq_on = cell_cache_on(c) && (mode == gls::MODE_JV || mode == gls::MODE_DIAG);
  if (cq_on) {
    const size_t need = cell_cache_size(c);
    if (c->cq.n != need) {
      GLS_TRY(c->cq.alloc(need));
      c->cq_valid = false;
    }
    if (mode == gls::MODE_JV && !c->cq_valid) {  // the diagonal pass at this state writes it
      c->diag_valid = false;
      GLS_TRY(ensure_diag(c));
    }
  }
  const bool split_jv = mode == gls::MODE_JV && split_jv_enabled(c);
  if (mode == gls::MODE_JV && !split_jv && !c->probe_local) GLS_TRY(dist_import(c, const_cast<double *>(v)));  // ghost values of v
  gls::OpParams P = make_params(c, mode != gls::MODE_RESIDUAL);
  if (mode == gls::MODE_JV && c->use_brick && c->use_qdata) {
    GLS_TRY(ensure_qdata(c));
    P.qd = c->qdata.p;
    mode = gls::MODE_JVQ;
  }
  bool lin_diag = false;  // brick path: the diagonal comes out of the linearization pass
  if (mode == gls::MODE_DIAG && c->use_brick && c->use_qdata) {
    const size_t nq = gls::brick_qdata_size(c->k, c->n_cells);
    if (c->qdata.n != nq) GLS_TRY(c->qdata.alloc(nq));
    P.qd = c->qdata.p;
    GLS_TRY(lin_f32_target(c, P));
    mode = gls::MODE_LIN;
    lin_diag = true;
  }
  if (mode == gls::MODE_JV && c->hang.on) {  // C v: hanging entries interpolated from their masters
    if (c->hang.vbuf.n != (size_t)c->n_dofs) GLS_TRY(c->hang.vbuf.alloc((size_t)c->n_dofs));
    if (c->hang.dmask.n == (size_t)c->n_dofs) {  // one pass: copy the free DoFs, interpolate the hanging ones
      HIP_TRY(gls::vec_copy_gather_set(c->hang.vbuf.p, v, c->hang.dmask.p, c->n_dofs, c->hang.dof.p, c->hang.ooff.p,
                                       c->hang.omaster.p, c->hang.ow.p, (int64_t)c->hang.dof.n, c->stream));
    } else {
      HIP_TRY(gls::vec_copy(c->hang.vbuf.p, v, c->n_dofs, c->stream));
      HIP_TRY(gls::vec_csr_gather_set(c->hang.vbuf.p, c->hang.vbuf.p, c->hang.dof.p, c->hang.ooff.p, c->hang.omaster.p,
                                      c->hang.ow.p, (int64_t)c->hang.dof.n, c->stream));
    }
    v = c->hang.vbuf.p;
  }
  P.v = v;
  P.y = y;
  P.hmask = c->hang.on ? c->hang.hmask.p : nullptr;
  const bool brick = c->use_brick && mode != gls::MODE_DIAG;
  const bool col = brick && c->use_colors;
  if (col) set_colors(c, P, y);  // every node is written exactly once: no zeroing, no slab sum
  else P.slab = brick ? brick_slab(c) : nullptr;
  if (!brick) {  // per-cell kernels: element vectors, then ordered per-node sums (no atomics)
    GLS_TRY(ensure_element_maps(c));
    P.ev = c->ev.p;
    if (cq_on) {
      P.cq = c->cq.p;
      P.cq_mode = mode == gls::MODE_DIAG ? 1 : 2;
    }
  }
  // adapted forest: the sibling-group bricks by the pencil kernel (J.v from the cached linearization; the
  // diagonal pass computes that cache), the other cells by the per-cell kernel (its cell list)
  const bool oct = c->oct.on && (mode == gls::MODE_JV || mode == gls::MODE_DIAG) && !brick;
  if (oct) {
    const size_t nq = gls::brick_qdata_size(c->k, 8 * c->oct.nb);
    if (c->qdata.n != nq) {
      GLS_TRY(c->qdata.alloc(nq));
      c->qd_valid = false;
      c->cq_valid = false;
    }
    if (mode == gls::MODE_JV && !c->qd_valid) GLS_TRY(oct_lin(c));  // linearization only, current state
    if (mode == gls::MODE_JV && c->oct.f32_next && !c->qd32_valid) {
      if (c->qdata32.n != c->qdata.n) GLS_TRY(c->qdata32.alloc(c->qdata.n));
      HIP_TRY(gls::vec_to_f32(c->qdata.p, c->qdata32.p, (int64_t)c->qdata.n, c->stream));
      c->qd32_valid = true;
    }
    P.cell_list = c->oct.rest.p;  // the per-cell kernel runs the cells outside the bricks only
    P.cell_list_n = c->oct.n_rest;
  }
  if (!col && !P.slab && !P.ev) HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * c->n_dofs, c->stream));
  {
    TimedLaunch t(c, mode == gls::MODE_JVQ ? (int)gls::MODE_JV : (lin_diag ? (int)gls::MODE_DIAG : mode));
    if (brick && split_jv && mode == gls::MODE_JVQ) {
      auto &D = c->dist;
      double *vv = const_cast<double *>(v);
      const int64_t voff = 3 * (int64_t)c->n_vnodes;
      if (D.on && !D.comm) {  // callback transport (GLS_SPLIT_DIST): the import completes first
        GLS_TRY(dist_import(c, vv));
      } else if (D.on) {  // ghost import of v on the exchange stream, ordered after v's producer
        HIP_TRY(hipEventRecord(D.ev_ready, c->stream));
        HIP_TRY(hipStreamWaitEvent(D.xstream, D.ev_ready, 0));
        HIP_TRY(gls::vec_pack_nodes(vv, D.send_nodes.p, D.n_send, voff, D.send_buf, D.xstream));
        if (rccl_exchange_on(c, 0, D.xstream) != 0) return set_err(GLS_ECOMM, "ghost import exchange failed");
        HIP_TRY(gls::vec_unpack_nodes(vv, D.recv_nodes.p, D.n_recv, voff, D.recv_buf, 0, D.xstream));
        HIP_TRY(hipEventRecord(D.ev_done, D.xstream));
      }
      gls::OpParams Q = P;  // interior bricks read no ghost value
      Q.subset = c->split.p + c->split_bnd;
      Q.subset_n = c->split_int;
      if (Q.subset_n > 0) HIP_TRY(gls::launch_brick_kernel(c->k, mode, Q, c->tables, c->stream));
      if (D.on && D.comm) HIP_TRY(hipStreamWaitEvent(c->stream, D.ev_done, 0));
      Q.subset = c->split.p;
      Q.subset_n = c->split_bnd;
      if (Q.subset_n > 0) HIP_TRY(gls::launch_brick_kernel(c->k, mode, Q, c->tables, c->stream));
    } else if (brick) {
      HIP_TRY(gls::launch_brick_kernel(c->k, mode, P, c->tables, c->stream));
    } else {
      // (the bricks' pencil launch forked onto a side stream, concurrent with this one and joined before the
      // gather, measured 1.0-1.4 ms per Newton step SLOWER on the 1.28 M-DoF octree line: the cross-stream event
      // pair costs more than the overlap of two ~20 us launches gains; profiles/r05_ab_octree_overlap.txt)
      HIP_TRY(gls::launch_cell_kernel(c->dim, c->k, c->kp, c->nq1d, mode, P, c->tables, c->stream));
      if (oct) {  // the bricks' cells: element vectors from the pencil kernel
        gls::OpParams Q = P;
        Q.cell_list = nullptr;
        Q.cell_list_n = 0;
        Q.y = nullptr;  // element vectors only
        Q.qd = c->qdata.p;
        Q.subset = c->oct.list.p;
        Q.subset_n = c->oct.nb;
        Q.brick_cell0 = c->oct.cell0.p;
        const bool f32 = mode == gls::MODE_JV && c->oct.f32_next;
        if (f32) Q.qdf = c->qdata32.p;
        HIP_TRY(gls::launch_pencil_ev(mode == gls::MODE_JV ? gls::MODE_JVQ : gls::MODE_LIN, Q, c->tables, c->stream, f32));
        if (mode == gls::MODE_DIAG) {
          c->qd_valid = true;
          c->qd32_valid = false;
        }
      }
    }
  }
  if (P.ev)
    HIP_TRY(gls::gather_element_vectors(y, c->ev.p, c->ev_voff.p, c->ev_vslot.p, c->n_vnodes, c->ev_poff.p,
                                        c->ev_pslot.p, c->n_pnodes, c->dim, c->stream));
  if (brick && !col && P.slab) {
    TimedLaunch t(c, 5);
    HIP_TRY(slab_sum(c, y));
  }
  // C^T y: the local cells' hanging rows onto their masters (masters across the partition are local
  // ghosts), then the ghost contributions to their owners (compress(add)); condensing the partial
  // rows before the export equals condensing the summed rows after it. (Folding this pass into the
  // element-vector gather measured slower on the 1.28 M-DoF octree line both ways: each master re-summing
  // its hanging rows' slots through their node maps +6.6 ms per Newton step, flattened (slot, weight) lists
  // per master DoF +1.6 ms -- the gather is bound by its dependent load chain, which either form lengthens;
  // profiles/r05_ab_cell_cache_fold.txt, r05_ab_condense_fold2.txt.)
  if (c->hang.on && (mode == gls::MODE_RESIDUAL || mode == gls::MODE_JV))
    HIP_TRY(gls::vec_csr_condense(y, c->hang.tm.p, c->hang.toff.p, c->hang.tdof.p, c->hang.tw.p,
                                  (int64_t)c->hang.tm.n, c->stream));
  if (!c->probe_local) GLS_TRY(dist_export_add(c, y));
  if (P.cq_mode == 1) {
    c->cq_valid = true;
    ++c->cq_epoch;
  }
  if (lin_diag) {  // the same launch stored the J.v linearization
    c->qd_valid = true;
    c->qd32_valid = P.qdf != nullptr;
    c->qd32_partial = P.qdf != nullptr && P.oseen;
  }
  return GLS_OK;
}

}  // namespace
namespace gls_impl {  // declared in gls_ctx.hpp
int ensure_diag(gls_ctx *c) {
  if (c->diag_valid) return GLS_OK;
  GLS_TRY(run_cell(c, gls::MODE_DIAG, nullptr, c->diag.p));
  if (c->dist.on) {  // ghost rows are not owned here: keep the Jacobi division finite
    const int64_t d = c->dim, nl = c->n_vnodes, no = c->dist.n_owned, npl = c->n_dofs - d * nl, nop = c->dist.n_owned_p;
    HIP_TRY(gls::vec_fill(c->diag.p + d * no, d * (nl - no), 1.0, c->stream));
    HIP_TRY(gls::vec_fill(c->diag.p + d * nl + nop, npl - nop, 1.0, c->stream));
  }
  c->diag_valid = true;
  return GLS_OK;
}
}  // namespace gls_impl
namespace {

int device_dot(gls_ctx *c, const double *a, const double *b, double *host_out) {
  return dist_multidot(c, a, 0, 1, b, host_out);
}

// Stream-ordered variants for GMRES (no host wait): the dots land in `out` (device), are reduced over
// ranks, and are copied to the pinned host buffer `hp` (read after the caller's next wait). The return
// value is the device address of the reduced dots, which the next projection reads as its
// coefficients directly (no host round trip, no H2D copy).
const double *reduce_dots_async(gls_ctx *c, const double *out, int nd, double *hp, int *err) {
  const double *res = out;
  *err = GLS_OK;
  if (c->dist.on) {
    if (hipMemcpyAsync(c->dist.red_buf, out, sizeof(double) * nd, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
      *err = set_err(GLS_EHIP, "reduce_dots_async: D2D copy");
      return nullptr;
    }
    if (c->dist.allreduce(c->dist.user, c->dist.red_buf, nd) != 0) {
      *err = set_err(GLS_ECOMM, "allreduce failed");
      return nullptr;
    }
    res = c->dist.red_buf;
  }
  if (hipMemcpyAsync(hp, res, sizeof(double) * nd, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
    *err = set_err(GLS_EHIP, "reduce_dots_async: D2H copy");
    return nullptr;
  }
  return res;
}
int multidot_async(gls_ctx *c, const double *A, int64_t lda, int nk, const double *w, double *out, double *hp,
                   const double **dev_res) {
  const int64_t n1 = c->dist.on ? (int64_t)c->dim * c->dist.n_owned : c->n_dofs;
  const int64_t off2 = c->dist.on ? (int64_t)c->dim * c->n_vnodes : 0;
  const int64_t n2 = c->dist.on ? c->dist.n_owned_p : 0;
  HIP_TRY(gls::vec_multidot2(A, lda, nk, w, n1, off2, n2, out, c->work.p, c->stream));
  int err;
  *dev_res = reduce_dots_async(c, out, nk, hp, &err);
  return err;
}
int multiaxpy_dots_async(gls_ctx *c, double *w, const double *V, int64_t lda, int nk, const double *h, bool dots,
                         double *out, double *hp, const double **dev_res, double scale = 1.0, double *x0 = nullptr,
                         const double *x0d = nullptr, double x0omega = 0.0) {
  const int64_t n1 = c->dist.on ? (int64_t)c->dim * c->dist.n_owned : c->n_dofs;
  const int64_t off2 = c->dist.on ? (int64_t)c->dim * c->n_vnodes : 0;
  const int64_t n2 = c->dist.on ? c->dist.n_owned_p : 0;
  HIP_TRY(gls::vec_multiaxpy_dots(w, V, lda, nk, h, 1.0, c->n_dofs, n1, off2, n2, dots, scale, out, c->work.p,
                                  c->stream, x0, x0d, x0omega));
  int err;
  *dev_res = reduce_dots_async(c, out, dots ? nk + 1 : 1, hp, &err);
  return err;
}

}  // namespace

extern "C" {

int gls_create(const gls_mesh_desc *d, gls_ctx **out) {
  if (!d || !out) return set_err(GLS_EINVAL, "null argument");
  *out = nullptr;
  const int nq1d = d->nq1d > 0 ? d->nq1d : d->k + 1;
  if (d->dim != 2 && d->dim != 3) return set_err(GLS_EINVAL, "dim must be 2 or 3");
  if (!gls::cell_kernel_supported(d->dim, d->k, d->kp, nq1d))
    return set_err(GLS_EINVAL, "unsupported element Q%d-Q%d (dim %d, QGauss %d)", d->k, d->kp, d->dim, nq1d);
  const bool mapped = d->map_degree > 0;
  if (d->n_cells < 0 || d->n_vnodes <= 0 || d->n_pnodes <= 0 || !d->cell_vnodes || (!mapped && !d->cell_h))
    return set_err(GLS_EINVAL, "incomplete mesh description");
  if (mapped && (d->map_degree > 2 || !d->cell_support))
    return set_err(GLS_EINVAL, "mapped cells: map_degree 1 or 2 with cell_support");
  if (d->kp != d->k && !d->cell_pnodes) return set_err(GLS_EINVAL, "cell_pnodes required when kp != k");
  if (d->srf && !d->cell_x0 && !mapped) return set_err(GLS_EINVAL, "srf requires cell_x0");
  std::unique_ptr<gls_ctx> c(new gls_ctx);
  c->dim = d->dim;
  c->k = d->k;
  c->kp = d->kp;
  c->nq1d = nq1d;
  c->n_cells = d->n_cells;
  c->n_vnodes = d->n_vnodes;
  c->n_pnodes = d->n_pnodes;
  c->nq = gls::ipow(nq1d, d->dim);
  c->n_dofs = (int64_t)d->dim * d->n_vnodes + d->n_pnodes;
  c->viscosity = d->viscosity;
  c->srf = d->srf;
  for (int i = 0; i < 3; ++i) c->omega[i] = d->omega[i];
  c->tables = make_tables(d->k, d->kp, nq1d);
  const int nv = gls::ipow(d->k + 1, d->dim), np = gls::ipow(d->kp + 1, d->dim);
  // validate indices
  for (int64_t i = 0; i < (int64_t)d->n_cells * nv; ++i)
    if (d->cell_vnodes[i] < 0 || d->cell_vnodes[i] >= d->n_vnodes) return set_err(GLS_EINVAL, "cell_vnodes out of range");
  if (d->cell_pnodes)
    for (int64_t i = 0; i < (int64_t)d->n_cells * np; ++i)
      if (d->cell_pnodes[i] < 0 || d->cell_pnodes[i] >= d->n_pnodes) return set_err(GLS_EINVAL, "cell_pnodes out of range");
  if (!d->cell_pnodes && d->n_pnodes != d->n_vnodes) return set_err(GLS_EINVAL, "n_pnodes != n_vnodes without cell_pnodes");

  GLS_TRY(c->cell_vnodes.upload(d->cell_vnodes, (size_t)d->n_cells * nv));
  c->use_brick = !mapped && detect_bricks(d, nq1d);
  if (c->use_brick) GLS_TRY(build_slab_map(c.get(), d));
  if (const char *e = std::getenv("GLS_JV_RECOMPUTE")) c->use_qdata = std::atoi(e) == 0;
  if (d->cell_pnodes) GLS_TRY(c->cell_pnodes.upload(d->cell_pnodes, (size_t)d->n_cells * np));
  std::vector<double> geo((size_t)d->n_cells * 4);
  const int nsup = mapped ? gls::ipow(d->map_degree + 1, d->dim) : 0;
  for (int cix = 0; cix < d->n_cells; ++cix) {
    double meas = 1.;
    if (mapped) {
      meas = corner_measure(d->dim, d->map_degree, d->cell_support + (size_t)cix * nsup * d->dim);
      if (!(meas > 0)) return set_err(GLS_EINVAL, "cell %d: non-positive measure (inverted cell)", cix);
      geo[cix * 4 + 0] = geo[cix * 4 + 1] = geo[cix * 4 + 2] = 1.0;
    } else {
      for (int e = 0; e < d->dim; ++e) {
        geo[cix * 4 + e] = d->cell_h[(size_t)cix * d->dim + e];
        meas *= geo[cix * 4 + e];
      }
      if (d->dim == 2) geo[cix * 4 + 2] = 1.0;
    }
    // element size for tau (gls_navier_stokes.cc:340-345)
    geo[cix * 4 + 3] = d->dim == 2 ? std::sqrt(4. * meas / M_PI) / d->k : std::pow(6 * meas / M_PI, 1. / 3.) / d->k;
  }
  GLS_TRY(c->geo.upload(geo.data(), geo.size()));
  if (mapped) {  // FEValues geometry per quadrature point (MappingQ(map_degree))
    c->map_degree = d->map_degree;
    c->host_support.assign(d->cell_support, d->cell_support + (size_t)d->n_cells * nsup * d->dim);
    std::vector<double> gq((size_t)d->n_cells * c->nq * gls::kGeo);
    for (int cix = 0; cix < d->n_cells; ++cix) {
      mapped_geometry(d->dim, d->map_degree, nq1d, d->cell_support + (size_t)cix * nsup * d->dim,
                      gq.data() + (size_t)cix * c->nq * gls::kGeo);
      for (int q = 0; q < c->nq; ++q)
        if (!(gq[((size_t)cix * c->nq + q) * gls::kGeo + gls::kGeoJxW] > 0))
          return set_err(GLS_EINVAL, "cell %d: non-positive Jacobian at quadrature point %d", cix, q);
    }
    GLS_TRY(c->gq.upload(gq.data(), gq.size()));
  } else {
    c->host_h.assign(d->cell_h, d->cell_h + (size_t)d->n_cells * d->dim);
    if (d->cell_x0) c->host_x0.assign(d->cell_x0, d->cell_x0 + (size_t)d->n_cells * d->dim);
  }
  if (d->cell_x0) {
    std::vector<double> x0((size_t)d->n_cells * 3, 0.);
    for (int cix = 0; cix < d->n_cells; ++cix)
      for (int e = 0; e < d->dim; ++e) x0[cix * 3 + e] = d->cell_x0[(size_t)cix * d->dim + e];
    GLS_TRY(c->x0.upload(x0.data(), x0.size()));
  }
  if (d->force_q) GLS_TRY(c->force_q.upload(d->force_q, (size_t)d->n_cells * c->nq * d->dim));
  std::vector<int64_t> con;
  if (d->vnode_mask) {
    GLS_TRY(c->vmask.upload(d->vnode_mask, (size_t)d->n_vnodes));
    for (int64_t n = 0; n < d->n_vnodes; ++n)
      for (int e = 0; e < d->dim; ++e)
        if ((d->vnode_mask[n] >> e) & 1) con.push_back(n * d->dim + e);
  }
  GLS_TRY(c->con_dofs.upload(con.data(), con.size()));
  GLS_TRY(c->diag.alloc(c->n_dofs));
  GLS_TRY(c->work.alloc(gls::multidot_work_size()));
  GLS_TRY(c->scal.alloc(64));
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
    return set_err(GLS_EHIP, "stream create failed");
  c->own_stream = true;
  HIP_TRY(hipDeviceSynchronize());
  *out = c.release();
  return GLS_OK;
}

int gls_destroy(gls_ctx *c) {
  if (!c) return GLS_OK;
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return GLS_OK;
}

int gls_set_stream(gls_ctx *c, void *s) {
  GLS_TRY(check_ctx(c));
  if (c->own_stream && c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  c->own_stream = false;
  c->stream = (hipStream_t)s;
  // multigrid levels run on the fine level's stream (the V-cycle interleaves their kernels)
  if (c->mg.on) {
    for (size_t l = 1; l < c->mg.lev.size(); ++l) GLS_TRY(gls_set_stream(c->mg.lev[l], s));
    // the replica's V-cycle is ordered with replica_gather / vec_pack_dofs on this stream
    if (c->mg.replica) GLS_TRY(gls_set_stream(c->mg.replica, s));
    if (c->mg.rep2) GLS_TRY(gls_set_stream(c->mg.rep2, s));
  }
  return GLS_OK;
}

int gls_uses_brick_kernels(const gls_ctx *c) { return c && c->use_brick ? 1 : 0; }

int gls_slab_lattice(const gls_ctx *c, int nb[3], int *tile) {
  if (!c || !c->use_brick || !c->use_slab) return 0;
  const bool cube = c->cube_nb1 > 0;
  if (!cube && c->box_nb[0] <= 0) return 0;
  for (int a = 0; a < 3 && nb; ++a) nb[a] = cube ? c->cube_nb1 : c->box_nb[a];
  if (tile) *tile = cube ? c->cube_nb1 : c->box_s;
  return cube ? 1 : 2;
}

int gls_quadrature_points(const gls_ctx *c, double *xq) {
  if (!c || !xq) return set_err(GLS_EINVAL, "null argument");
  const int dim = c->dim, nq = c->nq;
  if (c->map_degree > 0) {
    const int nsup = gls::ipow(c->map_degree + 1, dim);
    std::vector<double> g((size_t)nq * gls::kGeo);
    for (int cix = 0; cix < c->n_cells; ++cix) {
      mapped_geometry(dim, c->map_degree, c->nq1d, c->host_support.data() + (size_t)cix * nsup * dim, g.data());
      for (int q = 0; q < nq; ++q)
        for (int e = 0; e < dim; ++e) xq[((size_t)cix * nq + q) * dim + e] = g[(size_t)q * gls::kGeo + gls::kGeoX + e];
    }
    return GLS_OK;
  }
  if (c->host_x0.empty()) return set_err(GLS_EINVAL, "gls_quadrature_points: the mesh was created without cell_x0");
  for (int cix = 0; cix < c->n_cells; ++cix)
    for (int q = 0; q < nq; ++q) {
      const int qi[3] = {q % c->nq1d, (q / c->nq1d) % c->nq1d, q / (c->nq1d * c->nq1d)};
      for (int e = 0; e < dim; ++e)
        xq[((size_t)cix * nq + q) * dim + e] =
            c->host_x0[(size_t)cix * dim + e] + c->host_h[(size_t)cix * dim + e] * c->tables.xi[qi[e]];
    }
  return GLS_OK;
}

int gls_n_dofs(const gls_ctx *c, int64_t *n) {
  if (!c || !n) return set_err(GLS_EINVAL, "null argument");
  *n = c->n_dofs;
  return GLS_OK;
}

int gls_set_force(gls_ctx *c, const double *f) {
  GLS_TRY(check_ctx(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!f) {
    c->force_q.release();
  } else {
    GLS_TRY(c->force_q.upload(f, (size_t)c->n_cells * c->nq * c->dim));
  }
  c->diag_valid = false;
  c->ilu.valid = false;
  c->qd_valid = false;
  c->cq_valid = false;
  return GLS_OK;
}

int gls_set_viscosity(gls_ctx *c, double nu) {
  GLS_TRY(check_ctx(c));
  c->viscosity = nu;
  c->diag_valid = false;
  c->ilu.valid = false;
  c->qd_valid = false;
  c->cq_valid = false;
  return GLS_OK;
}

// assembleGLS preamble: gls_navier_stokes.cc:295-329 and the scheme branches :477-516, :530-533
int gls_set_time(gls_ctx *c, int scheme, const double ts[4]) {
  GLS_TRY(check_ctx(c));
  if (scheme < GLS_STEADY || scheme > GLS_SDIRK3_3) return set_err(GLS_EINVAL, "scheme %d", scheme);
  if (scheme != GLS_STEADY && (!ts || ts[0] == 0.)) return set_err(GLS_EINVAL, "time steps required");
  c->scheme = scheme;
  if (ts)
    for (int i = 0; i < 4; ++i) c->time_steps[i] = ts[i];
  if (!c->jf.on) c->mg.dirty = true;
  for (double &a : c->alpha) a = 0.;
  c->alpha_jac = 0.;
  c->sdt2 = 0.;
  c->n_hist = 0;
  if (scheme != GLS_STEADY) {
    const double sdt = 1. / ts[0];
    c->sdt2 = sdt * sdt;
  }
  if (scheme == GLS_BDF1 || scheme == GLS_BDF2 || scheme == GLS_BDF3) {
    const int order = scheme - GLS_BDF1 + 1;
    double a[6];
    GLS_TRY(gls_bdf_coefficients(order, ts, 4, a));
    for (int i = 0; i <= order; ++i) c->alpha[i] = a[i];
    c->alpha_jac = a[0];
    c->n_hist = order;
  } else if (is_sdirk(scheme)) {
    const bool three = scheme == GLS_SDIRK3 || scheme == GLS_SDIRK3_1 || scheme == GLS_SDIRK3_2 || scheme == GLS_SDIRK3_3;
    const int order = three ? 3 : 2;
    double t[12];
    GLS_TRY(gls_sdirk_coefficients(order, ts[0], t));
    int stage = 0;  // sdirk2 / sdirk3 (no stage) contribute no time term, like the reference
    if (scheme == GLS_SDIRK2_1 || scheme == GLS_SDIRK3_1) stage = 1;
    if (scheme == GLS_SDIRK2_2 || scheme == GLS_SDIRK3_2) stage = 2;
    if (scheme == GLS_SDIRK3_3) stage = 3;
    c->alpha_jac = t[0];
    if (stage > 0) {
      for (int i = 0; i <= stage; ++i) c->alpha[i] = t[(stage - 1) * (order + 1) + i];
      c->n_hist = stage;
    }
  }
  if (!c->jf.on) {  // a frozen Jacobian keeps its own time coefficients
    c->diag_valid = false;
    c->ilu.valid = false;
    c->qd_valid = false;
    c->cq_valid = false;
  }
  return GLS_OK;
}

int gls_set_state(gls_ctx *c, const double *u, const double *u1, const double *u2, const double *u3) {
  GLS_TRY(check_ctx(c));
  if (!u) return set_err(GLS_EINVAL, "u is null");
  c->bnorm2_of = nullptr;
  c->u = u;
  c->u1 = u1;
  c->u2 = u2;
  c->u3 = u3;
  if (!c->jf.on) {  // a frozen Jacobian stays at its snapshot (gls_freeze_jacobian)
    c->diag_valid = false;
    c->ilu.valid = false;
    c->qd_valid = false;
    c->cq_valid = false;
    c->mg.dirty = true;
  }
  // distributed: refresh the ghost values of the evaluation point (history vectors are imported
  // by the caller once per time step with gls_dist_import)
  return dist_import(c, const_cast<double *>(u));
}

// Jacobian snapshot for skip_newton (skip_newton_non_linear_solver.h:66-70, 126-130): freeze = 1
// copies the current state vectors and time coefficients; the Jacobian operators (J.v, diagonal,
// linearization, multigrid levels) stay at that snapshot while later gls_set_state / gls_set_time
// calls move only the residual. freeze = 0 releases it (everything is re-derived lazily).
int gls_freeze_jacobian(gls_ctx *c, int freeze) {
  GLS_TRY(check_ctx(c));
  auto &j = c->jf;
  if (!freeze) {
    if (j.on) {
      j.on = false;
      c->diag_valid = false;
      c->ilu.valid = false;
      c->qd_valid = false;
      c->cq_valid = false;
      c->mg.dirty = true;
    }
    return GLS_OK;
  }
  if (!c->u) return set_err(GLS_EINVAL, "gls_freeze_jacobian: gls_set_state was not called");
  if (j.on) return GLS_OK;  // already frozen at its snapshot
  const size_t n = (size_t)c->n_dofs;
  if (j.u.n != n) GLS_TRY(j.u.alloc(n));
  HIP_TRY(hipMemcpyAsync(j.u.p, c->u, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  const double *hs[3] = {c->u1, c->u2, c->u3};
  for (int h = 0; h < 3; ++h) {
    j.has[h] = hs[h] != nullptr && h < c->n_hist;
    if (!j.has[h]) continue;
    if (j.h[h].n != n) GLS_TRY(j.h[h].alloc(n));
    HIP_TRY(hipMemcpyAsync(j.h[h].p, hs[h], sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  }
  for (int i = 0; i < 4; ++i) {
    j.alpha[i] = c->alpha[i];
    j.ts[i] = c->time_steps[i];
  }
  j.alpha_jac = c->alpha_jac;
  j.sdt2 = c->sdt2;
  j.n_hist = c->n_hist;
  j.scheme = c->scheme;
  j.on = true;  // diag / linearization / multigrid computed so far belong to this very state
  return GLS_OK;
}

int gls_dist_import(gls_ctx *c, double *x) {
  GLS_TRY(check_ctx(c));
  return dist_import(c, x);
}

int gls_dist_attach(gls_ctx *c, int64_t n_owned_nodes, int n_nbrs, const int64_t *send_offsets,
                    const int32_t *send_nodes, const int64_t *recv_offsets, const int32_t *recv_nodes, double *send_buf,
                    double *recv_buf, double *red_buf, gls_exchange_fn xchg, gls_allreduce_fn allreduce, void *user) {
  GLS_TRY(check_ctx(c));
  if (c->dim != 3 || c->k != c->kp || c->cell_pnodes.p) return set_err(GLS_EINVAL, "distributed path: 3D Qk-Qk only");
  if (n_owned_nodes < 0 || n_owned_nodes > c->n_vnodes || n_nbrs < 0 || !xchg || !allreduce || !red_buf)
    return set_err(GLS_EINVAL, "gls_dist_attach: bad arguments");
  const int64_t ns = n_nbrs ? send_offsets[n_nbrs] : 0, nr = n_nbrs ? recv_offsets[n_nbrs] : 0;
  for (int64_t i = 0; i < ns; ++i)
    if (send_nodes[i] < 0 || send_nodes[i] >= n_owned_nodes) return set_err(GLS_EINVAL, "send node not owned");
  for (int64_t i = 0; i < nr; ++i)
    if (recv_nodes[i] < n_owned_nodes || recv_nodes[i] >= c->n_vnodes) return set_err(GLS_EINVAL, "recv node not a ghost");
  if ((ns && !send_buf) || (nr && !recv_buf)) return set_err(GLS_EINVAL, "exchange buffers missing");
  GLS_TRY(upload_export_order(c->dist, send_nodes, ns));
  GLS_TRY(c->dist.send_nodes.upload(send_nodes, (size_t)ns));
  GLS_TRY(c->dist.recv_nodes.upload(recv_nodes, (size_t)nr));
  c->dist.n_owned = n_owned_nodes;
  c->dist.n_owned_p = n_owned_nodes;
  c->dist.dofs = false;
  c->dist.width = 4;
  c->dist.n_send = ns;
  c->dist.n_recv = nr;
  c->dist.send_buf = send_buf;
  c->dist.recv_buf = recv_buf;
  c->dist.red_buf = red_buf;
  c->dist.xchg = xchg;
  c->dist.allreduce = allreduce;
  c->dist.user = user;
  c->dist.on = true;
  c->diag_valid = false;
  c->ilu.valid = false;
  c->qd_valid = false;
  c->cq_valid = false;
  if (c->use_brick && gls::brick_subset_supported(c->k)) {  // boundary / interior bricks (overlapped J.v)
    std::vector<char> flag((size_t)c->n_vnodes, 0);
    for (int64_t i = 0; i < ns; ++i) flag[(size_t)send_nodes[i]] = 1;
    for (int64_t i = 0; i < nr; ++i) flag[(size_t)recv_nodes[i]] = 1;
    GLS_TRY(build_brick_split(c, flag));
  }
  return GLS_OK;
}

int gls_dist_attach_dofs(gls_ctx *c, int64_t n_owned_vnodes, int64_t n_owned_pnodes, int n_nbrs,
                         const int64_t *send_offsets, const int32_t *send_dofs, const int64_t *recv_offsets,
                         const int32_t *recv_dofs, double *send_buf, double *recv_buf, double *red_buf,
                         gls_exchange_fn xchg, gls_allreduce_fn allreduce, void *user) {
  GLS_TRY(check_ctx(c));
  const int64_t nvd = (int64_t)c->dim * c->n_vnodes, npn = c->n_dofs - nvd;
  if (n_owned_vnodes < 0 || n_owned_vnodes > c->n_vnodes || n_owned_pnodes < 0 || n_owned_pnodes > npn || n_nbrs < 0 ||
      !xchg || !allreduce || !red_buf)
    return set_err(GLS_EINVAL, "gls_dist_attach_dofs: bad arguments");
  if (c->mg.on) return set_err(GLS_EINVAL, "gls_dist_attach_dofs: no multigrid");
  const int64_t ns = n_nbrs ? send_offsets[n_nbrs] : 0, nr = n_nbrs ? recv_offsets[n_nbrs] : 0;
  auto owned = [&](int64_t d) { return d < nvd ? d / c->dim < n_owned_vnodes : d - nvd < n_owned_pnodes; };
  for (int64_t i = 0; i < ns; ++i)
    if (send_dofs[i] < 0 || send_dofs[i] >= c->n_dofs || !owned(send_dofs[i])) return set_err(GLS_EINVAL, "send DoF not owned");
  for (int64_t i = 0; i < nr; ++i)
    if (recv_dofs[i] < 0 || recv_dofs[i] >= c->n_dofs || owned(recv_dofs[i])) return set_err(GLS_EINVAL, "recv DoF not a ghost");
  if ((ns && !send_buf) || (nr && !recv_buf)) return set_err(GLS_EINVAL, "exchange buffers missing");
  auto &D = c->dist;
  GLS_TRY(upload_export_order(D, send_dofs, ns));
  GLS_TRY(D.send_nodes.upload(send_dofs, (size_t)ns));
  GLS_TRY(D.recv_nodes.upload(recv_dofs, (size_t)nr));
  D.h_send.assign(send_dofs, send_dofs + ns);
  D.h_recv.assign(recv_dofs, recv_dofs + nr);
  D.h_soff.assign(1, 0);
  D.h_roff.assign(1, 0);
  if (n_nbrs > 0) {
    D.h_soff.assign(send_offsets, send_offsets + n_nbrs + 1);
    D.h_roff.assign(recv_offsets, recv_offsets + n_nbrs + 1);
  }
  D.dofs = true;
  D.width = 1;
  D.n_owned = n_owned_vnodes;
  D.n_owned_p = n_owned_pnodes;
  D.n_send = ns;
  D.n_recv = nr;
  D.send_buf = send_buf;
  D.recv_buf = recv_buf;
  D.red_buf = red_buf;
  D.xchg = xchg;
  D.allreduce = allreduce;
  D.user = user;
  D.on = true;
  c->diag_valid = false;
  c->ilu.valid = false;
  c->qd_valid = false;
  c->cq_valid = false;
  return GLS_OK;
}

int gls_residual(gls_ctx *c, double *rhs) {
  GLS_TRY(check_ctx(c));
  if (!rhs) return set_err(GLS_EINVAL, "rhs is null");
  c->bnorm2_of = nullptr;
  GLS_TRY(run_cell(c, gls::MODE_RESIDUAL, nullptr, rhs));
  HIP_TRY(gls::vec_set_indexed(rhs, c->con_dofs.p, nullptr, (int64_t)c->con_dofs.n, c->stream));
  return GLS_OK;
}

// assemble_matrix_and_rhs (gls_navier_stokes.cc:917-1000: assembleGLS<true>, the matrix and the rhs in
// one cell loop): on
// the Q2 brick path one pencil launch (MODE_RESLIN) computes the residual, the J.v linearization and
// the Jacobian diagonal at the current state (the residual's and the diagonal's node sums are bitwise
// those of the separate launches); elsewhere -- and with a frozen Jacobian, hanging nodes, colored or
// distributed launches, GLS_NO_RESLIN=1 -- the residual and the diagonal separately
int gls_residual_and_diagonal(gls_ctx *c, double *rhs, double *d) {
  GLS_TRY(check_ctx(c));
  if (!rhs) return set_err(GLS_EINVAL, "rhs is null");
  c->bnorm2_of = nullptr;
  if (!c->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  if (c->n_hist > 0 && !c->u1) return set_err(GLS_EINVAL, "scheme needs solution_m1");
  if (c->n_hist > 1 && !c->u2) return set_err(GLS_EINVAL, "scheme needs solution_m2");
  if (c->n_hist > 2 && !c->u3) return set_err(GLS_EINVAL, "scheme needs solution_m3");
  const bool fuse = !c->diag_valid && c->use_brick && c->use_qdata && c->use_slab && !c->use_colors && !c->hang.on &&
                    !c->dist.on && !c->jf.on && c->k == 2 && c->cube_nb1 > 0 && gls::pencil_enabled() &&
                    std::getenv("GLS_NO_RESLIN") == nullptr;
  if (fuse) {
    const size_t nq = gls::brick_qdata_size(c->k, c->n_cells);
    if (c->qdata.n != nq) GLS_TRY(c->qdata.alloc(nq));
    double *slab = brick_slab(c);
    if (!slab) return set_err(GLS_ENOMEM, "slab allocation failed");
    if (c->slab2.n != c->slab.n) GLS_TRY(c->slab2.alloc(c->slab.n));
    gls::OpParams P = make_params(c, true);
    P.qd = c->qdata.p;
    GLS_TRY(lin_f32_target(c, P));
    P.y = c->diag.p;
    P.slab = slab;
    P.res_y = rhs;
    P.res_slab = c->slab2.p;
    {
      TimedLaunch t(c, gls::MODE_DIAG);
      HIP_TRY(gls::launch_pencil_reslin(P, c->tables, c->stream));
    }
    {
      TimedLaunch t(c, 5);
      HIP_TRY(slab_sum_ex(c, c->slab2.p, nullptr, rhs, nullptr, nullptr, nullptr, 0.0, nullptr));
    }
    {
      TimedLaunch t(c, 5);
      HIP_TRY(slab_sum(c, c->diag.p));
    }
    HIP_TRY(gls::vec_set_indexed(rhs, c->con_dofs.p, nullptr, (int64_t)c->con_dofs.n, c->stream));
    c->qd_valid = true;
    c->qd32_valid = P.qdf != nullptr;
  c->qd32_partial = P.qdf != nullptr && P.oseen;
    c->diag_valid = true;
  } else {
    GLS_TRY(gls_residual(c, rhs));
    GLS_TRY(ensure_diag(c));
  }
  if (d && d != c->diag.p) HIP_TRY(gls::vec_copy(d, c->diag.p, c->n_dofs, c->stream));
  return GLS_OK;
}

int gls_jacobian_diagonal(gls_ctx *c, double *d) {
  GLS_TRY(check_ctx(c));
  GLS_TRY(ensure_diag(c));
  if (d && d != c->diag.p) HIP_TRY(gls::vec_copy(d, c->diag.p, c->n_dofs, c->stream));
  return GLS_OK;
}

int gls_jacobian_apply(gls_ctx *c, const double *v, double *y) {
  GLS_TRY(check_ctx(c));
  if (!v || !y || v == y) return set_err(GLS_EINVAL, "v/y null or aliased");
  if (c->con_dofs.n || c->dist.on) GLS_TRY(ensure_diag(c));  // (collective across ranks: on every rank)
  GLS_TRY(run_cell(c, gls::MODE_JV, v, y));
  HIP_TRY(gls::vec_gather_scale_set(y, c->diag.p, v, c->con_dofs.p, (int64_t)c->con_dofs.n, c->stream));
  return GLS_OK;
}

}  // extern "C"
namespace gls_impl {  // declared in gls_ctx.hpp
// the V-cycle's operator on level g: J.v in FP32 arithmetic from the FP32 linearization when the
// level smooths in mixed precision (brick path), else the FP64 gls_jacobian_apply. Same
// constraint handling (constrained rows D_c v) and ghost exchange as gls_jacobian_apply.
// full = false: u and tau suffice (the Oseen smoother operator); else every row of the FP32 copy
int ensure_qdata32(gls_ctx *g, bool full) {
  GLS_TRY(ensure_qdata(g));
  if (!g->qd32_valid || (full && g->qd32_partial)) {
    if (g->qdata32.n != g->qdata.n) GLS_TRY(g->qdata32.alloc(g->qdata.n));
    HIP_TRY(gls::vec_to_f32(g->qdata.p, g->qdata32.p, (int64_t)g->qdata.n, g->stream));
    g->qd32_valid = true;
    g->qd32_partial = false;
  }
  return GLS_OK;
}
// FP32 kernels write their brick-surface partial sums in FP32 (half the slab traffic; summed in FP64)
bool slab_f32() { return std::getenv("GLS_SLAB_F64") == nullptr; }
// rb != nullptr: y = rb - A v (the V-cycle's residual), fused into the kernels' stores on one rank.
// first_omega > 0 (only where first_sweep_fusable): v is not read but formed as the first damped-Jacobi
// sweep from 0, v = 0 + first_omega rb / D (mg_jacobi_update's arithmetic), in the J.v's gather and
// stored to v by the J.v (brick-interior nodes) and the slab sum (surface nodes). Opt-in
// (GLS_MG_FIRST_FUSE=1): bitwise the separate update, but measured slower at Q2 128^3 (99.5 vs 96.0 ms per
// Newton step, profiles/r04_ab_env_switches.txt: the gather's two extra FP64 loads and FP64 divisions per
// node cost the J.v more than the update pass it saves; with the restriction inside that J.v still no win,
// 79.5-79.9 vs 78.6-79.5 ms, profiles/fused_prolongation_ab.txt)
bool first_sweep_fusable(gls_ctx *g) {
  const char *e = std::getenv("GLS_MG_FIRST_FUSE");
  return e && std::atoi(e) != 0 && g->smooth_f32 && g->use_brick && g->use_qdata && !g->use_colors && !g->dist.on &&
         !g->hang.on && g->k == 2 && g->cube_nb1 > 0 && g->use_slab && gls::pencil_enabled() &&
         std::getenv("GLS_MG_NO_FUSE") == nullptr;
}
int jacobian_apply_f32(gls_ctx *g, const double *v, double *y, const double *rb, double first_omega, bool oseen) {
  if (!g->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  GLS_TRY(ensure_diag(g));
  GLS_TRY(ensure_qdata32(g, !oseen));
  GLS_TRY(dist_import(g, const_cast<double *>(v)));
  gls::OpParams P = make_params(g, true);
  P.qdf = g->qdata32.p;
  P.oseen = oseen ? 1 : 0;
  P.v = v;
  P.y = y;
  const bool col = g->use_colors;
  P.slab = col ? nullptr : brick_slab(g);
  const bool fuse_rb = rb && (P.slab || col) && !g->dist.on && gls::brick_fused_jacobi_supported(g->k) &&
                       std::getenv("GLS_MG_NO_FUSE") == nullptr;
  P.rb = fuse_rb ? rb : nullptr;
  P.slabf = P.slab && slab_f32() && gls::brick_fused_jacobi_supported(g->k) ? reinterpret_cast<float *>(P.slab)
                                                                             : nullptr;
  if (first_omega > 0.0) {
    if (!fuse_rb || !first_sweep_fusable(g)) return set_err(GLS_EINVAL, "fused first sweep not applicable");
    P.jx0 = const_cast<double *>(v);
    P.jd = g->diag.p;
    P.jomega = first_omega;
  }
  if (col) set_colors(g, P, y);
  if (!col && !P.slab) HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * g->n_dofs, g->stream));
  {
    TimedLaunch t(g, 4);
    HIP_TRY(gls::launch_brick_jv_f32(g->k, P, g->tables, g->stream));
  }
  if (P.slab) {
    TimedLaunch t(g, 5);
    HIP_TRY(slab_sum_ex(g, P.slab, P.slabf, y, nullptr, nullptr, P.jx0 ? g->diag.p : nullptr, P.jomega, P.rb, P.jx0));
  }
  GLS_TRY(dist_export_add(g, y));
  HIP_TRY(gls::vec_gather_scale_set(y, g->diag.p, v, g->con_dofs.p, (int64_t)g->con_dofs.n, g->stream, P.rb));
  if (rb && !fuse_rb) HIP_TRY(gls::vec_axpby(y, 1.0, rb, -1.0, g->n_dofs, g->stream));
  return GLS_OK;
}
// y = A v with the level's smoothing operator; rb != nullptr: y = rb - A v
int smoother_apply(gls_ctx *g, const double *v, double *y, const double *rb) {
  if (g->smooth_f32 && g->use_brick && g->use_qdata) return jacobian_apply_f32(g, v, y, rb, 0.0, g->smooth_oseen);
  g->oct.f32_next = g->smooth_f32 && g->oct.on;  // adapted forest: its bricks in FP32, the other cells FP64
  const int rc = gls_jacobian_apply(g, v, y);
  g->oct.f32_next = false;
  GLS_TRY(rc);
  if (rb) HIP_TRY(gls::vec_axpby(y, 1.0, rb, -1.0, g->n_dofs, g->stream));
  return GLS_OK;
}
// one ILU(0) smoothing sweep x <- x + M^-1 (b - A x) (M = the level's ILU(0), undamped; z: scratch)
static int ilu_sweep(gls_ctx *g, double *x, const double *b, double *y, double *z) {
  GLS_TRY(ensure_ilu(g));
  GLS_TRY(gls_jacobian_apply(g, x, y));
  HIP_TRY(gls::vec_axpby(y, 1.0, b, -1.0, g->n_dofs, g->stream));  // y = b - A x
  GLS_TRY(apply_ilu(g, y, z));
  HIP_TRY(gls::vec_axpy(x, 1.0, z, g->n_dofs, g->stream));
  return GLS_OK;
}
// one damped-Jacobi sweep x <- x + omega D^-1 (b - A x) with the smoother's operator A (constrained
// rows D_c x). Single rank on the brick path: fused into the J.v (brick-interior nodes) and the slab
// sum (brick-surface nodes), so A x is never stored; otherwise smoother_apply + mg_jacobi_update.
// pxc != nullptr (only where mg_fused_prolong_ok): the sweep starts from x + P pxc, the coarse correction of the
// next-coarser nested level interpolated in the J.v's gather; y (scratch) carries x + P pxc of the brick-surface
// nodes from the J.v to the slab sum.
int smoother_sweep(gls_ctx *g, double *x, const double *b, double *y, double omega, double *z, const double *pxc) {
  const bool nofuse = std::getenv("GLS_MG_NO_FUSE") != nullptr;
  const bool brick = g->use_brick && g->use_qdata && (g->use_colors || brick_slab(g)) && !g->dist.on &&
                     !g->hang.on && gls::brick_fused_jacobi_supported(g->k);
  if (pxc && ((z && g->ilu.on && !g->ilu.probe_only) || nofuse || !brick || !g->smooth_f32 || g->use_colors || g->cube_nb1 <= 0))
    return set_err(GLS_EINVAL, "fused prolongation not applicable");
  if (z && g->ilu.on && !g->ilu.probe_only) return ilu_sweep(g, x, b, y, z);
  if (g->vanka.smooth) return vanka_sweep(g, x, b, y, omega);
  if (nofuse || !brick) {
    GLS_TRY(smoother_apply(g, x, y));
    HIP_TRY(gls::mg_jacobi_update(x, b, y, g->diag.p, omega, g->n_dofs, 0, g->stream));
    return GLS_OK;
  }
  if (!g->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  GLS_TRY(ensure_diag(g));
  const bool f32 = g->smooth_f32;
  GLS_TRY(f32 ? ensure_qdata32(g, !g->smooth_oseen) : ensure_qdata(g));
  gls::OpParams P = make_params(g, true);
  P.v = x;
  P.y = x;
  P.jx = x;
  P.jb = b;
  P.jd = g->diag.p;
  P.jomega = omega;
  if (g->use_colors) {  // surface-node running sums in a scratch vector (x is updated in place)
    if (g->acc.n != (size_t)g->n_dofs) GLS_TRY(g->acc.alloc((size_t)g->n_dofs));
    set_colors(g, P, g->acc.p);
  } else {
    P.slab = brick_slab(g);
  }
  if (f32) {
    P.qdf = g->qdata32.p;
    P.oseen = g->smooth_oseen ? 1 : 0;
    P.slabf = P.slab && slab_f32() ? reinterpret_cast<float *>(P.slab) : nullptr;
    P.pxc = pxc;
    P.pxp = pxc ? y : nullptr;
    P.cube_nb1 = g->cube_nb1;
    TimedLaunch t(g, 4);
    HIP_TRY(pxc ? gls::launch_pencil_jv_prolong(P, g->tables, g->stream)
                : gls::launch_brick_jv_f32(g->k, P, g->tables, g->stream));
  } else {
    P.qd = g->qdata.p;
    TimedLaunch t(g, 1);
    HIP_TRY(gls::launch_brick_kernel(g->k, gls::MODE_JVQ, P, g->tables, g->stream));
  }
  if (g->use_colors) return GLS_OK;
  TimedLaunch t(g, 5);
  HIP_TRY(slab_sum_ex(g, P.slab, P.slabf, x, g->vmask.p, b, g->diag.p, omega, nullptr, nullptr, pxc ? y : nullptr));
  return GLS_OK;
}
}  // namespace gls_impl
extern "C" {

// y = A_s v with the operator the attached V-cycle smooths this level with (FP32 / Oseen per gls_mg_params)
int gls_mg_smoother_apply(gls_ctx *c, const double *v, double *y) {
  GLS_TRY(check_ctx(c));
  if (!v || !y || v == y) return set_err(GLS_EINVAL, "v/y null or aliased");
  return smoother_apply(c, v, y);
}

int gls_jacobian_apply_f32(gls_ctx *c, const double *v, double *y) {
  GLS_TRY(check_ctx(c));
  if (!v || !y || v == y) return set_err(GLS_EINVAL, "v/y null or aliased");
  if (!(c->use_brick && c->use_qdata)) return set_err(GLS_EINVAL, "FP32 J.v needs the 3D Qk-Qk brick path");
  return jacobian_apply_f32(c, v, y);
}

int gls_set_dirichlet(gls_ctx *c, int64_t n, const int64_t *dofs, const double *vals) {
  GLS_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!dofs || !vals))) return set_err(GLS_EINVAL, "dirichlet arrays");
  for (int64_t i = 0; i < n; ++i)
    if (dofs[i] < 0 || dofs[i] >= c->n_dofs) return set_err(GLS_EINVAL, "dirichlet dof out of range");
  HIP_TRY(hipStreamSynchronize(c->stream));
  GLS_TRY(c->dir_dofs.upload(dofs, (size_t)n));
  GLS_TRY(c->dir_vals.upload(vals, (size_t)n));
  return GLS_OK;
}

int gls_apply_dirichlet(gls_ctx *c, double *x) {
  GLS_TRY(check_ctx(c));
  HIP_TRY(gls::vec_set_indexed(x, c->dir_dofs.p, c->dir_vals.p, (int64_t)c->dir_dofs.n, c->stream));
  // across ranks the masters of the lines below may be ghosts: their owners' values first (on every
  // rank, whether or not it holds lines: the exchange is collective)
  if (c->dist.on && c->dist.dofs) GLS_TRY(dist_import(c, x));
  if (c->hang.on)  // hanging values from their masters (all masters: Dirichlet values included)
    HIP_TRY(gls::vec_csr_gather_set(x, x, c->hang.dof.p, c->hang.off.p, c->hang.master.p, c->hang.w.p,
                                    (int64_t)c->hang.dof.n, c->stream));
  if (!c->jf.on && (x == c->u || x == c->u1 || x == c->u2 || x == c->u3)) {  // the captured state changed
    c->diag_valid = false;
    c->ilu.valid = false;
    c->qd_valid = false;
    c->cq_valid = false;
    c->mg.dirty = true;
  }
  return GLS_OK;
}

}  // extern "C"
// sibling groups of an adapted forest's leaves that form 2x2x2 bricks: 8 consecutive cells (the forest's
// depth-first order keeps a complete family together, children x fastest) of equal extents whose node
// maps agree on the 5^3 brick lattice (a node shared by two cells sits at the same brick position in
// both). GLS_OCT_BRICKS=0: per-cell kernels only.
static int detect_oct_bricks(gls_ctx *c) {
  auto &O = c->oct;
  O = gls_ctx::Oct();
  const char *e = std::getenv("GLS_OCT_BRICKS");
  if ((e && std::atoi(e) == 0) || c->dim != 3 || c->k != 2 || c->kp != 2 || c->map_degree > 0 || c->dist.on ||
      c->cell_pnodes.p || c->host_h.empty() || !gls::pencil_enabled() || c->n_cells < 8)
    return GLS_OK;
  const int64_t nc = c->n_cells;
  std::vector<int32_t> cv((size_t)nc * 27);
  HIP_TRY(hipMemcpy(cv.data(), c->cell_vnodes.p, cv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> cell0;
  std::vector<char> in((size_t)nc, 0);
  int32_t lat[125];
  for (int64_t i = 0; i + 8 <= nc;) {
    bool ok = true;
    for (int ci = 1; ci < 8 && ok; ++ci)
      for (int d = 0; d < 3; ++d) ok = ok && c->host_h[(size_t)(i + ci) * 3 + d] == c->host_h[(size_t)i * 3 + d];
    for (int t = 0; t < 125 && ok; ++t) lat[t] = -1;
    for (int ci = 0; ci < 8 && ok; ++ci) {
      const int cx = ci & 1, cy = (ci >> 1) & 1, cz = ci >> 2;
      for (int a = 0; a < 27 && ok; ++a) {
        const int X = 2 * cx + a % 3, Y = 2 * cy + (a / 3) % 3, Z = 2 * cz + a / 9;
        int32_t &slot = lat[X + 5 * (Y + 5 * Z)];
        const int32_t nd = cv[(size_t)(i + ci) * 27 + a];
        if (slot < 0) slot = nd;
        else ok = slot == nd;
      }
    }
    if (ok) {  // 125 distinct nodes
      std::vector<int32_t> u(lat, lat + 125);
      std::sort(u.begin(), u.end());
      ok = std::adjacent_find(u.begin(), u.end()) == u.end();
    }
    if (ok) {
      cell0.push_back((int32_t)i);
      for (int ci = 0; ci < 8; ++ci) in[(size_t)(i + ci)] = 1;
      i += 8;
    } else {
      ++i;
    }
  }
  if (cell0.empty()) return GLS_OK;
  std::vector<int32_t> rest;
  for (int64_t q = 0; q < nc; ++q)
    if (!in[(size_t)q]) rest.push_back((int32_t)q);
  std::vector<int32_t> list(cell0.size());
  for (size_t b = 0; b < list.size(); ++b) list[b] = (int32_t)b;
  GLS_TRY(O.cell0.upload(cell0.data(), cell0.size()));
  GLS_TRY(O.list.upload(list.data(), list.size()));
  O.n_rest = (int)rest.size();
  if (rest.empty()) rest.push_back(0);  // (no per-cell launch when n_rest == 0)
  GLS_TRY(O.rest.upload(rest.data(), rest.size()));
  O.nb = (int)cell0.size();
  O.on = true;
  return GLS_OK;
}
extern "C" {
int gls_forest_bricks(const gls_ctx *c) { return c && c->oct.on ? c->oct.nb : 0; }

int gls_set_hanging(gls_ctx *c, int64_t n, const int64_t *dofs, const int64_t *off, const int64_t *masters,
                    const double *w) {
  GLS_TRY(check_ctx(c));
  if (n < 0 || (n > 0 && (!dofs || !off || !masters || !w))) return set_err(GLS_EINVAL, "gls_set_hanging: arrays");
  if (c->mg.on) return set_err(GLS_EINVAL, "hanging constraints: no multigrid");
  if (c->dist.on && !c->dist.dofs) return set_err(GLS_EINVAL, "hanging constraints across ranks: gls_dist_attach_dofs");
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int dim = c->dim;
  const int64_t N = c->n_dofs, nvd = (int64_t)dim * c->n_vnodes;
  std::vector<uint8_t> vm((size_t)c->n_vnodes, 0);
  if (c->vmask.p) HIP_TRY(hipMemcpy(vm.data(), c->vmask.p, (size_t)c->n_vnodes, hipMemcpyDeviceToHost));
  auto dirichlet = [&](int64_t d) { return d < nvd && ((vm[(size_t)(d / dim)] >> (d % dim)) & 1); };
  std::vector<char> is_h((size_t)N, 0);
  if (n > 0 && off[0] != 0) return set_err(GLS_EINVAL, "gls_set_hanging: offsets[0] != 0");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t d = dofs[i];
    if (d < 0 || d >= N || off[i + 1] < off[i]) return set_err(GLS_EINVAL, "gls_set_hanging: line %lld", (long long)i);
    if (dirichlet(d)) return set_err(GLS_EINVAL, "hanging DoF %lld carries a Dirichlet mask bit", (long long)d);
    if (is_h[(size_t)d]) return set_err(GLS_EINVAL, "hanging DoF %lld listed twice", (long long)d);
    is_h[(size_t)d] = 1;
  }
  const int64_t nm = n ? off[n] : 0;
  for (int64_t j = 0; j < nm; ++j)
    if (masters[j] < 0 || masters[j] >= N || is_h[(size_t)masters[j]])
      return set_err(GLS_EINVAL, "gls_set_hanging: master %lld out of range or hanging itself", (long long)masters[j]);
  // operator lines (closed zero_constraints: Dirichlet masters drop out) and their transpose
  std::vector<int64_t> ooff{0}, omas, cnt((size_t)N + 1, 0);
  std::vector<double> ow;
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = off[i]; j < off[i + 1]; ++j)
      if (!dirichlet(masters[j])) {
        omas.push_back(masters[j]);
        ow.push_back(w[j]);
        ++cnt[(size_t)masters[j] + 1];
      }
    ooff.push_back((int64_t)omas.size());
  }
  std::vector<int64_t> tm, toff{0};
  std::vector<int64_t> start((size_t)N + 1, 0);
  for (int64_t m = 0; m < N; ++m) {
    start[(size_t)m + 1] = start[(size_t)m] + cnt[(size_t)m + 1];
    if (cnt[(size_t)m + 1]) {
      tm.push_back(m);
      toff.push_back(start[(size_t)m + 1]);
    }
  }
  std::vector<int64_t> tdof(omas.size()), fill(start.begin(), start.end() - 1);
  std::vector<double> tw(omas.size());
  for (int64_t i = 0; i < n; ++i)  // lines in order: each master sums its hanging rows in a fixed order
    for (int64_t j = ooff[(size_t)i]; j < ooff[(size_t)i + 1]; ++j) {
      const int64_t slot = fill[(size_t)omas[(size_t)j]]++;
      tdof[(size_t)slot] = dofs[i];
      tw[(size_t)slot] = ow[(size_t)j];
    }
  c->hang.h_dof.assign(dofs, dofs + n);
  c->hang.h_off.assign(off, off + n + 1);
  c->hang.h_master.assign(masters, masters + nm);
  if (n == 0) c->hang.h_off.assign(1, 0);
  std::vector<uint8_t> hm((size_t)c->n_vnodes, 0), dm((size_t)N, 0);
  std::vector<int64_t> con;  // zero_constraints: Dirichlet + hanging
  for (int64_t d = 0; d < N; ++d) {
    if (is_h[(size_t)d] && d < nvd) hm[(size_t)(d / dim)] |= (uint8_t)(1u << (d % dim));
    dm[(size_t)d] = is_h[(size_t)d] ? 1 : 0;
    if (is_h[(size_t)d] || dirichlet(d)) con.push_back(d);
  }
  auto &h = c->hang;
  GLS_TRY(h.dof.upload(dofs, (size_t)n));
  GLS_TRY(h.off.upload(off, (size_t)(n ? n + 1 : 0)));
  GLS_TRY(h.master.upload(masters, (size_t)nm));
  GLS_TRY(h.w.upload(w, (size_t)nm));
  GLS_TRY(h.ooff.upload(ooff.data(), n ? ooff.size() : 0));
  GLS_TRY(h.omaster.upload(omas.data(), omas.size()));
  GLS_TRY(h.ow.upload(ow.data(), ow.size()));
  GLS_TRY(h.tm.upload(tm.data(), tm.size()));
  GLS_TRY(h.toff.upload(toff.data(), tm.empty() ? 0 : toff.size()));
  GLS_TRY(h.tdof.upload(tdof.data(), tdof.size()));
  GLS_TRY(h.tw.upload(tw.data(), tw.size()));
  GLS_TRY(h.hmask.upload(hm.data(), hm.size()));
  GLS_TRY(h.dmask.upload(dm.data(), dm.size()));
  GLS_TRY(c->con_dofs.upload(con.data(), con.size()));
  h.on = n > 0;
  c->use_brick = false;  // mixed cell sizes: the general per-cell kernels
  c->use_slab = false;
  c->use_colors = false;
  c->diag_valid = false;
  c->ilu.valid = false;
  c->qd_valid = false;
  c->cq_valid = false;
  return detect_oct_bricks(c);
}

namespace {
// z = M^{-1} v : Jacobi, assembled ILU(0) or a multigrid V-cycle when attached. x0_ready (only where
// mg_fine_first_producer allows): z already holds the V-cycle's first sweep from 0 on v
int apply_prec(gls_ctx *c, const double *v, double *z, bool x0_ready = false) {
  if (c->mg.on && c->mg.rep_csr) return mg_vcycle_rep2(c, v, z);
  if (c->mg.on) return mg_vcycle(c, 0, v, z, x0_ready);
  if (c->ilu.on && !c->ilu.probe_only) return apply_ilu(c, v, z);
  HIP_TRY(gls::vec_div(z, v, c->diag.p, c->n_dofs, c->stream));
  return GLS_OK;
}
}  // namespace

int gls_apply_preconditioner(gls_ctx *c, const double *v, double *z) {
  GLS_TRY(check_ctx(c));
  if (!v || !z || v == z) return set_err(GLS_EINVAL, "v/z null or aliased");
  GLS_TRY(ensure_diag(c));
  if (c->mg.on) GLS_TRY(mg_prepare(c));
  GLS_TRY(ensure_ilu(c));
  return apply_prec(c, v, z);
}


// --------------------------------------------------------------------------------------------
// GMRES(m), right preconditioned (Jacobi, the V-cycle or the assembled ILU). Orthogonalisation:
// Gram-corrected classical Gram–Schmidt (one projection pass per iteration, see the loop) or, with
// gls_linear_params.orthogonalization = GLS_ORTHO_CGS2, classical Gram–Schmidt with one DGKS re-orthogonalisation
// pass; fused multi-dot /
// multi-axpy kernels (one pass over the Krylov basis per Gram–Schmidt sweep). Stopping test on the unpreconditioned residual
// ||b - A x|| <= max(rel*||b||, abs) (deal.II SolverControl / AztecOO AZ_noscaled).
// --------------------------------------------------------------------------------------------
// BiCGStab (solve_system_BiCGStab, gls_navier_stokes.cc:1293-1340: TrilinosWrappers::SolverBicgstab =
// AztecOO AZ_bicgstab with the same ILU, here with whatever preconditioner gls_solve_linear applies),
// right preconditioned (van der Vorst's BiCGStab on A M^-1, x = M^-1 y), so the recursively updated
// residual is the unpreconditioned b - A x the reference's tolerance rule tests:
// ||r|| <= max(rel ||b||, abs). One iteration = one BiCGStab step (two operator applications), as
// AztecOO counts. Breakdown (rho or (rhat, v) or (t, t) vanishing) stops with the current iterate.
static int solve_bicgstab(gls_ctx *c, const double *b, double *x, gls_linear_params *prm) {
  const int64_t n = c->n_dofs;
  hipStream_t s = c->stream;
  // work vectors: r, rhat, p, v, phat, shat, t (the GMRES basis storage when it is large enough)
  double *w[7];
  if (c->krylov.p && c->krylov.n >= (size_t)7 * n) {
    for (int i = 0; i < 7; ++i) w[i] = c->krylov.p + (int64_t)i * n;
  } else {
    if (c->bicg.n != (size_t)7 * n) GLS_TRY(c->bicg.alloc((size_t)7 * n));
    for (int i = 0; i < 7; ++i) w[i] = c->bicg.p + (int64_t)i * n;
  }
  double *r = w[0], *rh = w[1], *p = w[2], *v = w[3], *ph = w[4], *sh = w[5], *t = w[6];
  double bn2;
  GLS_TRY(device_dot(c, b, b, &bn2));
  const double tol = std::max(prm->relative_residual * std::sqrt(bn2), prm->minimum_residual);
  HIP_TRY(gls::vec_fill(x, n, 0.0, s));
  HIP_TRY(gls::vec_copy(r, b, n, s));
  HIP_TRY(gls::vec_copy(rh, b, n, s));
  HIP_TRY(gls::vec_fill(p, n, 0.0, s));
  HIP_TRY(gls::vec_fill(v, n, 0.0, s));
  double res = std::sqrt(bn2), rho = 1.0, alpha = 1.0, omega = 1.0;
  int it = 0;
  bool converged = res <= tol;
  while (!converged && it < prm->max_iterations) {
    double rho1;
    GLS_TRY(device_dot(c, rh, r, &rho1));
    if (rho1 == 0.0 || omega == 0.0) break;  // breakdown
    const double beta = (rho1 / rho) * (alpha / omega);
    rho = rho1;
    // p = r + beta (p - omega v)
    HIP_TRY(gls::vec_axpy(p, -omega, v, n, s));
    HIP_TRY(gls::vec_axpby(p, 1.0, r, beta, n, s));
    GLS_TRY(apply_prec(c, p, ph));
    GLS_TRY(gls_jacobian_apply(c, ph, v));
    double rhv;
    GLS_TRY(device_dot(c, rh, v, &rhv));
    if (rhv == 0.0) break;
    alpha = rho / rhv;
    HIP_TRY(gls::vec_axpy(r, -alpha, v, n, s));  // r <- s = r - alpha v
    HIP_TRY(gls::vec_axpy(x, alpha, ph, n, s));  // x += alpha M^-1 p
    ++it;
    double sn2;
    GLS_TRY(device_dot(c, r, r, &sn2));
    res = std::sqrt(sn2);
    if (res <= tol) {
      converged = true;
      break;
    }
    GLS_TRY(apply_prec(c, r, sh));
    GLS_TRY(gls_jacobian_apply(c, sh, t));
    double tt, ts;
    GLS_TRY(device_dot(c, t, t, &tt));
    GLS_TRY(device_dot(c, t, r, &ts));
    if (tt == 0.0) break;
    omega = ts / tt;
    HIP_TRY(gls::vec_axpy(x, omega, sh, n, s));  // x += omega M^-1 s
    HIP_TRY(gls::vec_axpy(r, -omega, t, n, s));  // r = s - omega t
    double rn2;
    GLS_TRY(device_dot(c, r, r, &rn2));
    res = std::sqrt(rn2);
    converged = res <= tol;
    if (getenv("GLS_GMRES_VERBOSE") && (it % 10 == 0 || it == 1))
      printf("  bicgstab it %d  res %.6e  (tol %.3e)\n", it, res, tol);
  }
  if (converged && prm->true_residual) {
    GLS_TRY(gls_jacobian_apply(c, x, t));
    HIP_TRY(gls::vec_axpby(t, 1.0, b, -1.0, n, s));
    double rn2;
    GLS_TRY(device_dot(c, t, t, &rn2));
    res = std::sqrt(rn2);
  }
  prm->iterations = it;
  prm->final_residual = res;
  if (!converged) return set_err(GLS_ENOCONV, "BiCGStab: %d iterations, residual %.3e > %.3e", it, res, tol);
  return GLS_OK;
}

int gls_solve_linear(gls_ctx *c, const double *b, double *x, gls_linear_params *prm) {
  GLS_TRY(check_ctx(c));
  if (!b || !x || !prm) return set_err(GLS_EINVAL, "null argument");
  const double *const bnorm2_of = c->bnorm2_of;  // consumed by this solve, whichever way it ends
  c->bnorm2_of = nullptr;
  const int m = prm->restart > 0 ? std::min(prm->restart, 200) : 30;
  const int64_t n = c->n_dofs;
  if (c->krylov_m != m || !c->krylov.p) {
    GLS_TRY(c->krylov.alloc((size_t)(m + 1) * n));
    GLS_TRY(c->coef.alloc((size_t)m + 8));
    if (c->scal.n < (size_t)m + 8) GLS_TRY(c->scal.alloc((size_t)m + 8));
    if (c->scal2.n < (size_t)m + 8) GLS_TRY(c->scal2.alloc((size_t)m + 8));
    if (c->hpin_n < 3 * ((size_t)m + 8)) {
      if (c->hpin) HIP_TRY(hipHostFree(c->hpin));
      c->hpin = nullptr;
      c->hpin_n = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->hpin), sizeof(double) * 3 * ((size_t)m + 8)));
      c->hpin_n = 3 * ((size_t)m + 8);
    }
    c->krylov_m = m;
  }
  if (!c->tmp1.p) {
    GLS_TRY(c->tmp1.alloc(n));
    GLS_TRY(c->tmp2.alloc(n));
  }
  GLS_TRY(ensure_diag(c));
  if (c->mg.on) GLS_TRY(mg_prepare(c));
  GLS_TRY(ensure_ilu(c));
  if (prm->method == GLS_LIN_BICGSTAB) return solve_bicgstab(c, b, x, prm);
  if (prm->method != GLS_LIN_GMRES) return set_err(GLS_EINVAL, "linear solver method %d unknown", prm->method);
  // with the V-cycle, keep Z = M^-1 V (flexible-GMRES storage): the update x += Z y then needs no
  // extra preconditioner application per restart cycle
  const bool keepz = c->mg.on;
  if (keepz && c->zbasis.n != (size_t)m * n) GLS_TRY(c->zbasis.alloc((size_t)m * n));
  double *V = c->krylov.p, *z = c->tmp1.p, *r = c->tmp2.p;
  hipStream_t s = c->stream;
  // ||b||^2: Newton's, when it just formed it from this vector with the same reduction (bitwise the dot below)
  double bnorm2 = c->bnorm2_val;
  if (bnorm2_of != b || std::getenv("GLS_GMRES_NO_NORM_REUSE") != nullptr) GLS_TRY(device_dot(c, b, b, &bnorm2));
  const double tol = std::max(prm->relative_residual * std::sqrt(bnorm2), prm->minimum_residual);
  // x = 0: with the Z basis the first update writes x = Z y without reading it (x_zero), and the first
  // restart cycle starts from r = b itself (no copy)
  bool x_zero = keepz;
  if (!keepz) HIP_TRY(gls::vec_fill(x, n, 0.0, s));
  const double *rcur = b;
  double beta = std::sqrt(bnorm2);
  int it = 0;
  std::vector<double> H((size_t)(m + 1) * m), cs(m), sn(m), g(m + 1), hc2(m + 2), y(m);
  // Gram-corrected single-pass orthogonalisation (default; prm->orthogonalization = GLS_ORTHO_CGS2: classical
  // Gram-Schmidt with the DGKS second pass); Gm: measured off-diagonal part of V^T V of the current restart cycle
  const bool gram = prm->orthogonalization != GLS_ORTHO_CGS2;
  int ortho_repairs = 0;
  // test knobs (read per call): GLS_GMRES_REPAIR_TOL (default 1e-8; 0 repairs every column) and
  // GLS_GMRES_REPAIR_MEASURED=1 (the repair pass always normalises by the measured norm)
  const double repair_tol = std::getenv("GLS_GMRES_REPAIR_TOL") ? std::atof(std::getenv("GLS_GMRES_REPAIR_TOL")) : 1e-8;
  const bool repair_measured = std::getenv("GLS_GMRES_REPAIR_MEASURED") != nullptr;
  // GLS_GMRES_FULL_LAST_COLUMN=1 (read per call): project (and repair) the column at which the solve converges
  // too, although nothing reads v_{j+1} then (A/B runs and tests)
  const char *fle = std::getenv("GLS_GMRES_FULL_LAST_COLUMN");
  const bool full_last = fle && std::atoi(fle) != 0;
  std::vector<double> hcol((size_t)m + 2);
  // the projection that writes v_{j+1} also stores the next V-cycle's first sweep from 0 into its x, Z's slot
  // j + 1 (x0d: the fine level's diagonal; nullptr: the cycle launches the update itself)
  const double *x0d = nullptr;
  double x0omega = 0.;
  if (keepz) GLS_TRY(mg_fine_first_producer(c, &x0d, &x0omega));
  bool x0_ready = false;  // Z's slot j holds that sweep for column j
  std::vector<double> Gm((size_t)(m + 1) * (m + 1), 0.0);
  bool converged = beta <= tol;
  const bool lverbose = std::getenv("GLS_ILU_VERBOSE") != nullptr;
  while (!converged && it < prm->max_iterations) {
    if (lverbose) std::printf("gmres: it %d residual %.6e (tol %.3e)\n", it, beta, tol);
    HIP_TRY(gls::vec_axpby(V, 1.0 / beta, rcur, 0.0, n, s));
    std::fill(Gm.begin(), Gm.end(), 0.);
    std::fill(g.begin(), g.end(), 0.);
    g[0] = beta;
    int j = 0;
    double res = beta;
    x0_ready = false;
    for (; j < m && it < prm->max_iterations; ++j) {
      double *vj = V + (int64_t)j * n, *w = V + (int64_t)(j + 1) * n;
      double *zj = keepz ? c->zbasis.p + (int64_t)j * n : z;
      GLS_TRY(apply_prec(c, vj, zj, x0_ready));
      x0_ready = false;
      double *x0 = x0d && j + 1 < m && j + 1 <= 8 ? c->zbasis.p + (int64_t)(j + 1) * n : nullptr;
      GLS_TRY(gls_jacobian_apply(c, zj, w));
      // h = V[0..j]^T w and ||w||^2 in one pass. The Gram-Schmidt passes are chained on the stream:
      // each projection reads the previous pass's dots from device memory (scal / scal2 alternate),
      // the host copies arrive in pinned memory, and the host waits once per pass pair (after the
      // projection, and after the DGKS correction when it is taken) instead of once per pass.
      double *hp1 = c->hpin, *hp2 = c->hpin + (m + 8), *hp3 = c->hpin + 2 * (m + 8);
      const double *hdev = nullptr, *h2dev = nullptr, *h3dev = nullptr;
      GLS_TRY(multidot_async(c, V, n, j + 2, w, c->scal.p, hp1, &hdev));
      double wn2, wnorm, wnorm0;
      bool normalized = false;  // w already scaled to v_{j+1} (H(j+1, j) set) by the fused DGKS pass
      bool done = false;        // the Gram-corrected single projection below handled this column
      bool rotated = false;     // the column converged before its projection: H, cs, sn, g already rotated
      if (gram) {
        // Gram-corrected classical Gram-Schmidt: ONE projection pass with h = (2I - G) h1, where
        // h1 = V^T w and G = V^T V (unit diagonal, off-diagonal part Gm measured by the previous
        // projections' fused dots) -- the first-order inverse of G, so w - V h is orthogonal to the
        // basis up to O(|G - I|^2) and rounding, as after CGS2's second pass, without that pass over
        // V. The projection also normalises (est^2 = |w|^2 - 2 h.h1 + h^T G h) and returns V^T v_{j+1}
        // (the next column of Gm) and |v_{j+1}|^2; a DGKS pass repairs the rare column whose measured
        // orthogonality or norm is off by more than 1e-8 (catastrophic cancellation).
        HIP_TRY(hipStreamSynchronize(s));
        const double wn0sq = std::max(hp1[j + 1], 0.0);
        wnorm0 = std::sqrt(wn0sq);
        auto G = [&](int a, int b) { return Gm[(size_t)std::min(a, b) * (m + 1) + std::max(a, b)]; };
        double *hc = hp3;
        for (int i = 0; i <= j; ++i) {
          double t = hp1[i];
          for (int k = 0; k <= j; ++k)
            if (k != i) t -= G(i, k) * hp1[k];
          hc[i] = t;
        }
        double q = wn0sq;
        for (int i = 0; i <= j; ++i) q += hc[i] * hc[i] - 2.0 * hc[i] * hp1[i];
        for (int i = 0; i <= j; ++i)
          for (int k = i + 1; k <= j; ++k) q += 2.0 * hc[i] * hc[k] * G(i, k);
        const bool qok = q > 1e-20 * wn0sq && q > 0.;
        const double est = qok ? std::sqrt(q) : 0.;
        // hc and est are this column of H before any repair: rotate a copy and form the residual estimate before
        // the projection is launched. On the column at which the solve converges nothing reads v_{j+1} (the update
        // x += Z y follows), so its projection, its repair pass and its Gram column are skipped and the rotated
        // copy is committed here (rotated: the Givens code below does not run again for this column)
        if (qok && !full_last) {
          for (int i = 0; i <= j; ++i) hcol[i] = hc[i];
          hcol[j + 1] = est;
          for (int i = 0; i < j; ++i) {
            const double a = hcol[i], bb = hcol[i + 1];
            hcol[i] = cs[i] * a + sn[i] * bb;
            hcol[i + 1] = -sn[i] * a + cs[i] * bb;
          }
          const double a = hcol[j], bb = hcol[j + 1];
          const double rr = std::hypot(a, bb);
          const double csj = rr > 0 ? a / rr : 1.0, snj = rr > 0 ? bb / rr : 0.0;
          if (std::fabs(-snj * g[j]) <= tol) {
            for (int i = 0; i < j; ++i) H[(size_t)i * m + j] = hcol[i];
            H[(size_t)j * m + j] = rr;
            H[(size_t)(j + 1) * m + j] = 0.;
            cs[j] = csj;
            sn[j] = snj;
            g[j + 1] = -snj * g[j];
            g[j] = csj * g[j];
            wnorm = est;
            normalized = done = rotated = true;
            if (std::getenv("GLS_GMRES_VERBOSE")) printf("  gmres: column %d converges, its projection is skipped\n", j);
          }
        }
        if (rotated) {
        } else if (qok) {
          HIP_TRY(hipMemcpyAsync(c->coef.p, hc, sizeof(double) * (j + 1), hipMemcpyHostToDevice, s));
          if (j + 1 <= 8) {
            GLS_TRY(multiaxpy_dots_async(c, w, V, n, j + 1, c->coef.p, true, c->scal2.p, hp2, &h2dev, 1.0 / est, x0, x0d,
                                         x0omega));
            x0_ready = x0 != nullptr;
          } else {
            HIP_TRY(gls::vec_multiaxpy(w, V, n, j + 1, c->coef.p, 1.0, n, s));
            HIP_TRY(gls::vec_scale(w, 1.0 / est, n, s));
            GLS_TRY(multidot_async(c, V, n, j + 2, w, c->scal2.p, hp2, &h2dev));
          }
          HIP_TRY(hipStreamSynchronize(s));
          for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = hc[i];
          H[(size_t)(j + 1) * m + j] = est;
          double gmax = 0., gg = 0.;
          for (int i = 0; i <= j; ++i) {
            gmax = std::max(gmax, std::fabs(hp2[i]));
            gg += hp2[i] * hp2[i];
          }
          const double nrm2 = hp2[j + 1];
          const double est2sq = nrm2 - gg;  // |v - V g|^2 if V were exactly orthonormal
          if (gmax > repair_tol || std::fabs(nrm2 - 1.0) > repair_tol) {
            // repair pass v' = (v - V g) / s: H column += est g, H(j+1, j) = est s. The first-order
            // estimate s = sqrt(|v|^2 - |g|^2) is used only when the cancellation leaves it well
            // above rounding (est2sq > 1e-4); otherwise the pass runs unscaled and s is the MEASURED
            // norm of its result. Either way the measured |v'|^2 returned by the pass decides: a
            // vector off unit length by more than 1e-8 is rescaled (with its H entry and Gram
            // column), and a vanishing one is a breakdown (the Krylov space is exhausted).
            const bool use_est = est2sq > 1e-4 && !repair_measured;
            const double est2 = use_est ? std::sqrt(est2sq) : 1.0;
            for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] += est * hp2[i];
            if (j + 1 <= 8) {
              GLS_TRY(multiaxpy_dots_async(c, w, V, n, j + 1, h2dev, true, c->scal.p, hp1, &hdev, 1.0 / est2, x0, x0d,
                                           x0omega));
            } else {
              HIP_TRY(gls::vec_multiaxpy(w, V, n, j + 1, h2dev, 1.0, n, s));
              if (use_est) HIP_TRY(gls::vec_scale(w, 1.0 / est2, n, s));
              GLS_TRY(multidot_async(c, V, n, j + 2, w, c->scal.p, hp1, &hdev));
            }
            HIP_TRY(hipStreamSynchronize(s));
            const double nn = std::max(hp1[j + 1], 0.0);  // measured |v'|^2
            double sc = 1.0;                               // v_{j+1} = v' / sc
            if (nn <= 1e-28 * (use_est ? 1.0 : std::max(nrm2, 1e-300))) {
              sc = 0.0;  // breakdown: w lies in span(V) to rounding
              x0_ready = false;
            } else if (!use_est || std::fabs(nn - 1.0) > 1e-8) {
              sc = std::sqrt(nn);
              HIP_TRY(gls::vec_scale(w, 1.0 / sc, n, s));
              x0_ready = false;  // w changed after the pass that stored x0: the cycle runs its own update
            }
            H[(size_t)(j + 1) * m + j] = est * est2 * sc;
            for (int i = 0; i <= j; ++i) Gm[(size_t)i * (m + 1) + j + 1] = sc > 0. ? hp1[i] / sc : 0.;
            ++ortho_repairs;
          } else {
            for (int i = 0; i <= j; ++i) Gm[(size_t)i * (m + 1) + j + 1] = hp2[i];
          }
          wnorm = H[(size_t)(j + 1) * m + j];
          normalized = done = true;
        }
      }
      if (done) {
      } else if (j + 1 <= 8) {
        // projection fused with the DGKS dots and the norm: one pass over V instead of three
        GLS_TRY(multiaxpy_dots_async(c, w, V, n, j + 1, hdev, true, c->scal2.p, hp2, &h2dev));
        HIP_TRY(hipStreamSynchronize(s));
        wnorm0 = std::sqrt(std::max(hp1[j + 1], 0.0));
        for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = hp1[i];
        std::copy(hp2, hp2 + j + 2, hc2.begin());
        wnorm = std::sqrt(std::max(hc2[j + 1], 0.0));
        if (wnorm < 0.7071 * wnorm0) {  // DGKS re-orthogonalisation with the dots of the fused pass
          for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] += hc2[i];
          // ||w''||^2 = ||w'||^2 - |V^T w'|^2 (V orthonormal): the correction pass also normalises,
          // v_{j+1} = w'' / est, and H(j+1, j) = est keeps A z_j = V H exactly (|v_{j+1}| = 1 + O(eps))
          double h2 = 0.;
          for (int i = 0; i <= j; ++i) h2 += hc2[i] * hc2[i];
          const double est2 = wnorm * wnorm - h2;
          if (est2 > 0.25 * wnorm * wnorm && est2 > 0.) {
            const double est = std::sqrt(est2);
            GLS_TRY(multiaxpy_dots_async(c, w, V, n, j + 1, h2dev, false, c->scal.p, hp3, &h3dev, 1.0 / est));
            HIP_TRY(hipStreamSynchronize(s));
            wn2 = hp3[0];
            H[(size_t)(j + 1) * m + j] = est;
            normalized = true;
            wnorm = est * std::sqrt(std::max(wn2, 0.0));
          } else {
            GLS_TRY(multiaxpy_dots_async(c, w, V, n, j + 1, h2dev, false, c->scal.p, hp3, &h3dev));
            HIP_TRY(hipStreamSynchronize(s));
            wn2 = hp3[0];
            wnorm = std::sqrt(std::max(wn2, 0.0));
          }
        }
      } else {
        HIP_TRY(gls::vec_multiaxpy(w, V, n, j + 1, hdev, 1.0, n, s));
        GLS_TRY(multidot_async(c, w, 0, 1, w, c->scal2.p, hp2, &h2dev));
        HIP_TRY(hipStreamSynchronize(s));
        wnorm0 = std::sqrt(std::max(hp1[j + 1], 0.0));
        for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] = hp1[i];
        wn2 = hp2[0];
        wnorm = std::sqrt(std::max(wn2, 0.0));
        if (wnorm < 0.7071 * wnorm0) {  // DGKS re-orthogonalisation
          GLS_TRY(multidot_async(c, V, n, j + 1, w, c->scal.p, hp1, &hdev));
          HIP_TRY(gls::vec_multiaxpy(w, V, n, j + 1, hdev, 1.0, n, s));
          GLS_TRY(multidot_async(c, w, 0, 1, w, c->scal2.p, hp2, &h2dev));
          HIP_TRY(hipStreamSynchronize(s));
          for (int i = 0; i <= j; ++i) H[(size_t)i * m + j] += hp1[i];
          wn2 = hp2[0];
          wnorm = std::sqrt(std::max(wn2, 0.0));
        }
      }
      if (!normalized) {
        H[(size_t)(j + 1) * m + j] = wnorm;
        if (wnorm > 0) HIP_TRY(gls::vec_scale(w, 1.0 / wnorm, n, s));
      }
      // Givens
      if (!rotated) {
        for (int i = 0; i < j; ++i) {
          const double a = H[(size_t)i * m + j], bb = H[(size_t)(i + 1) * m + j];
          H[(size_t)i * m + j] = cs[i] * a + sn[i] * bb;
          H[(size_t)(i + 1) * m + j] = -sn[i] * a + cs[i] * bb;
        }
        const double a = H[(size_t)j * m + j], bb = H[(size_t)(j + 1) * m + j];
        const double rr = std::hypot(a, bb);
        cs[j] = rr > 0 ? a / rr : 1.0;
        sn[j] = rr > 0 ? bb / rr : 0.0;
        H[(size_t)j * m + j] = rr;
        H[(size_t)(j + 1) * m + j] = 0.;
        g[j + 1] = -sn[j] * g[j];
        g[j] = cs[j] * g[j];
      }
      res = std::fabs(g[j + 1]);
      ++it;
      if (getenv("GLS_GMRES_VERBOSE") && (it % 10 == 0 || it == 1))
        printf("  gmres it %d  res %.6e  (tol %.3e)\n", it, res, tol);
      if (res <= tol || wnorm == 0.) { ++j; break; }
    }
    // back substitution and update x += M^{-1} V y
    const int kdim = j;
    for (int i = kdim - 1; i >= 0; --i) {
      double s_ = g[i];
      for (int l = i + 1; l < kdim; ++l) s_ -= H[(size_t)i * m + l] * y[l];
      y[i] = H[(size_t)i * m + i] != 0. ? s_ / H[(size_t)i * m + i] : 0.;
    }
    HIP_TRY(hipMemcpyAsync(c->coef.p, y.data(), sizeof(double) * kdim, hipMemcpyHostToDevice, s));
    if (keepz) {
      HIP_TRY(gls::vec_multiaxpy(x, c->zbasis.p, n, kdim, c->coef.p, -1.0, n, s, x_zero));  // x += Z y
      x_zero = false;
    } else {
      HIP_TRY(gls::vec_fill(r, n, 0.0, s));
      HIP_TRY(gls::vec_multiaxpy(r, V, n, kdim, c->coef.p, -1.0, n, s));  // r = V y
      GLS_TRY(apply_prec(c, r, z));
      HIP_TRY(gls::vec_axpy(x, 1.0, z, n, s));
    }
    // converged on the recurrence estimate: done (as deal.II's SolverGMRES, which recomputes the
    // true residual only at a restart)
    if (res <= tol) {
      beta = res;
      converged = true;
      if (prm->true_residual) {  // the caller asked for ||b - A x|| instead of the recurrence estimate
        GLS_TRY(gls_jacobian_apply(c, x, r));
        HIP_TRY(gls::vec_axpby(r, 1.0, b, -1.0, n, s));
        double rn2;
        GLS_TRY(device_dot(c, r, r, &rn2));
        beta = std::sqrt(rn2);
      }
      break;
    }
    // true residual r = b - A x
    GLS_TRY(gls_jacobian_apply(c, x, r));
    HIP_TRY(gls::vec_axpby(r, 1.0, b, -1.0, n, s));
    rcur = r;
    double rn2;
    GLS_TRY(device_dot(c, r, r, &rn2));
    beta = std::sqrt(rn2);
    converged = beta <= tol;
    if (beta == 0.) break;
  }
  if (x_zero) HIP_TRY(gls::vec_fill(x, n, 0.0, s));  // no update was made (b below the tolerance)
  prm->iterations = it;
  prm->final_residual = beta;
  if (ortho_repairs && std::getenv("GLS_GMRES_VERBOSE")) printf("  gmres: %d orthogonality repair passes\n", ortho_repairs);
  if (!converged) return set_err(GLS_ENOCONV, "GMRES: %d iterations, residual %.3e > %.3e", it, beta, tol);
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// NewtonNonLinearSolver::solve (include/core/newton_non_linear_solver.h:74-139), one template
// driving any "physics" with the PhysicsSolver hooks (include/core/physics_solver.h:64-102).
// --------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

struct NewtonStats {
  int outer = 0, linear = 0, residuals = 0;
  double final_res = 0.;
};

// SkipNewtonNonLinearSolver::solve (include/core/skip_newton_non_linear_solver.h:54-131): the
// Jacobian (and its preconditioner) is assembled only when consecutive_iters == 0, on the initial
// step or when forced, and only in the first outer iteration; every later iteration reuses it.
template <class Phys>
int skip_newton_template(Phys &ph, double tolerance, int max_iterations, int verbosity, int skip_iterations,
                         bool is_initial_step, bool force_matrix_renewal, int &consecutive, NewtonStats &st) {
  double current_res = 1.0, last_res = 1.0;
  int outer = 0;
  bool assembly_needed = consecutive == 0 || is_initial_step || force_matrix_renewal;
  while (current_res > tolerance && outer < max_iterations) {
    GLS_TRY(ph.evaluation_point_from_present());
    if (assembly_needed) {
      GLS_TRY(ph.assemble_matrix_and_rhs());
      ++st.residuals;
    } else if (outer == 0) {
      GLS_TRY(ph.assemble_rhs());
      ++st.residuals;
    }
    if (outer == 0) {
      GLS_TRY(ph.rhs_norm(current_res));
      last_res = current_res;
    }
    if (verbosity) printf("Newton iteration: %d  - Residual:  %g\n", outer, current_res);
    int lin_it = 0;
    GLS_TRY(ph.solve_linear_system(lin_it));  // renewed_matrix = assembly_needed: reused otherwise
    st.linear += lin_it;
    for (double alpha = 1.0; alpha > 1e-3; alpha *= 0.5) {
      GLS_TRY(ph.line_point(alpha));
      GLS_TRY(ph.assemble_rhs());
      ++st.residuals;
      GLS_TRY(ph.rhs_norm(current_res));
      if (verbosity) printf("\t\talpha = %6g res = %g\n", alpha, current_res);
      if (current_res < 0.9 * last_res || last_res < tolerance) break;
    }
    GLS_TRY(ph.present_from_evaluation_point());
    last_res = current_res;
    ++outer;
    assembly_needed = false;
  }
  if (!force_matrix_renewal) consecutive = (consecutive + 1) % std::max(skip_iterations, 1);
  st.outer = outer;
  st.final_res = current_res;
  return GLS_OK;
}

template <class Phys>
int newton_template(Phys &ph, double tolerance, int max_iterations, int verbosity, NewtonStats &st) {
  double current_res = 1.0, last_res = 1.0;
  int outer = 0;
  while (current_res > tolerance && outer < max_iterations) {
    GLS_TRY(ph.evaluation_point_from_present());          // evaluation_point = present_solution
    GLS_TRY(ph.assemble_matrix_and_rhs());
    ++st.residuals;
    if (outer == 0) {
      GLS_TRY(ph.rhs_norm(current_res));
      last_res = current_res;
    }
    if (verbosity) printf("Newton iteration: %d  - Residual:  %g\n", outer, current_res);
    int lin_it = 0;
    GLS_TRY(ph.solve_linear_system(lin_it));
    st.linear += lin_it;
    for (double alpha = 1.0; alpha > 1e-3; alpha *= 0.5) {
      GLS_TRY(ph.line_point(alpha));  // local_eval = present + alpha*update; apply_constraints; eval = local_eval
      GLS_TRY(ph.assemble_rhs());
      ++st.residuals;
      GLS_TRY(ph.rhs_norm(current_res));
      if (verbosity) printf("\t\talpha = %6g res = %g\n", alpha, current_res);
      if (current_res < 0.9 * last_res || last_res < tolerance) break;
    }
    GLS_TRY(ph.present_from_evaluation_point());  // present_solution = evaluation_point
    last_res = current_res;
    ++outer;
  }
  st.outer = outer;
  st.final_res = current_res;
  return GLS_OK;
}

// one TimerOutput::Scope of the reference (gls_navier_stokes.cc:921, 1028, 1165, 1274): host wall
// time of the section with the context stream drained on entry and exit (the reference's sections
// are synchronous host code); no cost while the timer is off
struct SectionScope {
  gls_ctx *c;
  int s;
  std::chrono::steady_clock::time_point t0;
  SectionScope(gls_ctx *c_, int s_) : c(c_), s(s_) {
    if (c->sec_on) {
      (void)hipStreamSynchronize(c->stream);
      t0 = std::chrono::steady_clock::now();
    }
  }
  ~SectionScope() {
    if (!c->sec_on) return;
    (void)hipStreamSynchronize(c->stream);
    c->sec_t[s] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++c->sec_n[s];
  }
};

// GLS physics on device vectors (the GLSNavierStokesSolver side of the plugin API)
struct DevicePhysics {
  gls_ctx *c;
  double *present, *eval, *update, *rhs;
  const double *u1, *u2, *u3;
  gls_linear_params lin;
  int verbosity;
  bool skip = false;  // skip_newton: the Jacobian is frozen between assemblies (gls_freeze_jacobian)
  int linear_failures = 0;
  int evaluation_point_from_present() {
    // the state IS present (no copy): the assembly reads it, the line search writes eval; the frozen-
    // Jacobian renewal (skip) re-states eval, so it keeps the reference's copy
    if (!skip) return gls_set_state(c, present, u1, u2, u3);
    HIP_TRY(gls::vec_copy(eval, present, c->n_dofs, c->stream));
    return gls_set_state(c, eval, u1, u2, u3);
  }
  int assemble_matrix_and_rhs() {  // matrix-free: residual + the Jacobian diagonal at this state
    SectionScope t(c, GLS_SEC_ASSEMBLE_SYSTEM);
    if (skip) {  // renew the frozen Jacobian at this evaluation point
      GLS_TRY(gls_freeze_jacobian(c, 0));
      GLS_TRY(gls_set_state(c, eval, u1, u2, u3));
    }
    GLS_TRY(gls_residual_and_diagonal(c, rhs, nullptr));
    return skip ? gls_freeze_jacobian(c, 1) : GLS_OK;
  }
  int assemble_rhs() {
    SectionScope t(c, GLS_SEC_ASSEMBLE_RHS);
    return gls_residual(c, rhs);
  }
  int rhs_norm(double &r) {
    double r2;
    GLS_TRY(device_dot(c, rhs, rhs, &r2));
    c->bnorm2_of = rhs;  // the solve that follows takes it (cleared when rhs is evaluated again)
    c->bnorm2_val = r2;
    r = std::sqrt(r2);
    return GLS_OK;
  }
  int solve_linear_system(int &its) {
    gls_linear_params lp = lin;
    if (c->mg.on) {  // preconditioner setup first (setup_ILU / setup_AMG, gls_navier_stokes.cc:1165, 1182)
      SectionScope t(c, GLS_SEC_SETUP_GMG);
      GLS_TRY(ensure_diag(c));
      GLS_TRY(mg_prepare(c));
    } else if (c->ilu.on && !c->ilu.probe_only) {
      SectionScope t(c, GLS_SEC_SETUP_ILU);
      GLS_TRY(ensure_diag(c));
      GLS_TRY(ensure_ilu(c));
    }
    SectionScope t(c, GLS_SEC_SOLVE_LINEAR);
    const int rc = gls_solve_linear(c, rhs, update, &lp);
    if (rc < 0 && rc != GLS_ENOCONV) return rc;
    if (rc == GLS_ENOCONV) {
      ++linear_failures;
      if (verbosity) printf("  -Iterative solver did not converge: %d steps, residual %g\n", lp.iterations, lp.final_residual);
    }
    its = lp.iterations;
    if (verbosity) printf("  -Iterative solver took : %d steps \n", lp.iterations);
    // zero_constraints.distribute(solution): constrained entries of the update are 0
    HIP_TRY(gls::vec_set_indexed(update, c->con_dofs.p, nullptr, (int64_t)c->con_dofs.n, c->stream));
    return GLS_OK;
  }
  int line_point(double alpha) {
    HIP_TRY(gls::vec_waxpy(eval, present, alpha, update, c->n_dofs, c->stream));  // eval = present + alpha update
    GLS_TRY(gls_apply_dirichlet(c, eval));  // nonzero_constraints.distribute
    return gls_set_state(c, eval, u1, u2, u3);
  }
  int present_from_evaluation_point() {
    HIP_TRY(gls::vec_copy(present, eval, c->n_dofs, c->stream));
    return GLS_OK;
  }
};

// the reference's fake physics (tests/core/non_linear_test_system_01.h:50-129)
struct KatPhysics {
  double present[2] = {1., 0.}, eval[2] = {0, 0}, update[2] = {0, 0}, rhs[2] = {0, 0};
  double J[2][2] = {{0, 0}, {0, 0}};
  int evaluation_point_from_present() { eval[0] = present[0]; eval[1] = present[1]; return GLS_OK; }
  int assemble_matrix_and_rhs() {
    J[0][0] = 2 * eval[0]; J[0][1] = 1; J[1][0] = 0; J[1][1] = 2;
    return assemble_rhs();
  }
  int assemble_rhs() {
    rhs[0] = -(eval[0] * eval[0] + eval[1]);
    rhs[1] = -(2 * eval[1] + 3);
    return GLS_OK;
  }
  int rhs_norm(double &r) { r = std::sqrt(rhs[0] * rhs[0] + rhs[1] * rhs[1]); return GLS_OK; }
  int solve_linear_system(int &its) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    if (det == 0.) return set_err(GLS_EINVAL, "singular KAT Jacobian");
    update[0] = (rhs[0] * J[1][1] - J[0][1] * rhs[1]) / det;
    update[1] = (J[0][0] * rhs[1] - J[1][0] * rhs[0]) / det;
    its = 1;
    return GLS_OK;
  }
  int line_point(double a) { eval[0] = present[0] + a * update[0]; eval[1] = present[1] + a * update[1]; return GLS_OK; }
  int present_from_evaluation_point() { present[0] = eval[0]; present[1] = eval[1]; return GLS_OK; }
};

}  // namespace

extern "C" {

int gls_newton_solve(gls_ctx *c, double *present, const double *u1, const double *u2, const double *u3,
                     gls_newton_params *prm) {
  GLS_TRY(check_ctx(c));
  if (!present || !prm) return set_err(GLS_EINVAL, "null argument");
  const int64_t n = c->n_dofs;
  if (!c->tmp3.p) {
    GLS_TRY(c->tmp3.alloc(n));  // evaluation_point
    GLS_TRY(c->tmp4.alloc(n));  // newton_update
    GLS_TRY(c->tmp5.alloc(n));  // system_rhs
  }
  DevicePhysics ph{c, present, c->tmp3.p, c->tmp4.p, c->tmp5.p, u1, u2, u3, prm->lin, prm->verbosity};
  NewtonStats st;
  if (prm->solver == GLS_SKIP_NEWTON) {
    ph.skip = true;
    GLS_TRY(skip_newton_template(ph, prm->tolerance, prm->max_iterations, prm->verbosity, prm->skip_iterations,
                                 prm->is_initial_step != 0, prm->force_matrix_renewal != 0, c->skip_consecutive, st));
  } else {
    GLS_TRY(gls_freeze_jacobian(c, 0));
    GLS_TRY(newton_template(ph, prm->tolerance, prm->max_iterations, prm->verbosity, st));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->bnorm2_of = nullptr;
  prm->newton_iterations = st.outer;
  prm->linear_iterations = st.linear;
  prm->residual_evaluations = st.residuals;
  prm->final_residual = st.final_res;
  prm->linear_failures = ph.linear_failures;
  return GLS_OK;
}

int gls_section_timing(gls_ctx *c, int enable) {
  GLS_TRY(check_ctx(c));
  c->sec_on = enable != 0;
  for (int i = 0; i < GLS_N_SECTIONS; ++i) {
    c->sec_t[i] = 0.;
    c->sec_n[i] = 0;
  }
  return GLS_OK;
}
int gls_section_get(const gls_ctx *c, int section, double *seconds, int *calls) {
  if (!c) return set_err(GLS_EINVAL, "null context");
  if (section < 0 || section >= GLS_N_SECTIONS) return set_err(GLS_EINVAL, "section %d", section);
  if (seconds) *seconds = c->sec_t[section];
  if (calls) *calls = c->sec_n[section];
  return GLS_OK;
}

// Newton KAT (tests/core/newton_non_linear_solver_01.cc: tol 1e-8, max 10 iterations)
int gls_newton_selftest(double xo[2]) {
  if (!xo) return set_err(GLS_EINVAL, "null");
  KatPhysics ph;
  NewtonStats st;
  GLS_TRY(newton_template(ph, 1e-8, 10, 0, st));
  xo[0] = ph.present[0];
  xo[1] = ph.present[1];
  return GLS_OK;
}

// SkipNewton KAT (tests/core/skip_newton_non_linear_solver_01.cc: tol 1e-8, max 10 iterations,
// skip iterations as given; solve_non_linear_system(steady, true, true))
int gls_skip_newton_selftest(int skip_iterations, double xo[2]) {
  if (!xo || skip_iterations < 1) return set_err(GLS_EINVAL, "gls_skip_newton_selftest arguments");
  KatPhysics ph;
  NewtonStats st;
  int consecutive = 0;
  GLS_TRY(skip_newton_template(ph, 1e-8, 10, 0, skip_iterations, true, true, consecutive, st));
  xo[0] = ph.present[0];
  xo[1] = ph.present[1];
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// hyper_cube + refine_global, Morton (z-order) cells, lexicographic nodes
// --------------------------------------------------------------------------------------------
int gls_mesh_hyper_cube_sizes(int dim, int n, int k, int kp, int pmask, int64_t *nc, int64_t *nv, int64_t *np) {
  if ((dim != 2 && dim != 3) || n <= 0 || k <= 0 || kp <= 0) return set_err(GLS_EINVAL, "mesh args");
  int64_t c = 1, v = 1, p = 1;
  for (int d = 0; d < dim; ++d) {
    const bool per = (pmask >> d) & 1;
    c *= n;
    v *= (int64_t)k * n + (per ? 0 : 1);
    p *= (int64_t)kp * n + (per ? 0 : 1);
  }
  if (nc) *nc = c;
  if (nv) *nv = v;
  if (np) *np = p;
  return GLS_OK;
}

int gls_mesh_hyper_cube(int dim, int n, int k, int kp, double lo, double hi, int pmask, int32_t *cv, int32_t *cp,
                        double *x0, double *h) {
  int64_t nc, nv, np;
  GLS_TRY(gls_mesh_hyper_cube_sizes(dim, n, k, kp, pmask, &nc, &nv, &np));
  if (nv > INT32_MAX || np > INT32_MAX) return set_err(GLS_EINVAL, "mesh too large for int32 node ids");
  int L = 0;
  while ((1 << L) < n) ++L;
  const double hc = (hi - lo) / n;
  int vsh[3], psh[3];
  for (int d = 0; d < 3; ++d) {
    const bool per = (pmask >> d) & 1;
    vsh[d] = k * n + (per ? 0 : 1);
    psh[d] = kp * n + (per ? 0 : 1);
  }
  const int nvl = gls::ipow(k + 1, dim), npl = gls::ipow(kp + 1, dim);
  int64_t cell = 0;
  const int64_t total = (int64_t)1 << (dim * L);
  for (int64_t mcode = 0; mcode < total; ++mcode) {
    int ijk[3] = {0, 0, 0};
    for (int b = 0; b < L; ++b)
      for (int d = 0; d < dim; ++d) ijk[d] |= (int)((mcode >> (b * dim + d)) & 1) << b;
    bool inside = true;
    for (int d = 0; d < dim; ++d) inside = inside && ijk[d] < n;
    if (!inside) continue;
    for (int a = 0; a < nvl; ++a) {
      int loc[3] = {a % (k + 1), (a / (k + 1)) % (k + 1), a / ((k + 1) * (k + 1))};
      int64_t id = 0, stride = 1;
      for (int d = 0; d < dim; ++d) {
        id += (int64_t)((ijk[d] * k + loc[d]) % vsh[d]) * stride;
        stride *= vsh[d];
      }
      cv[cell * nvl + a] = (int32_t)id;
    }
    if (cp) {
      for (int a = 0; a < npl; ++a) {
        int loc[3] = {a % (kp + 1), (a / (kp + 1)) % (kp + 1), a / ((kp + 1) * (kp + 1))};
        int64_t id = 0, stride = 1;
        for (int d = 0; d < dim; ++d) {
          id += (int64_t)((ijk[d] * kp + loc[d]) % psh[d]) * stride;
          stride *= psh[d];
        }
        cp[cell * npl + a] = (int32_t)id;
      }
    }
    for (int d = 0; d < dim; ++d) {
      if (x0) x0[cell * dim + d] = lo + ijk[d] * hc;
      if (h) h[cell * dim + d] = hc;
    }
    ++cell;
  }
  return cell == nc ? GLS_OK : set_err(GLS_EINVAL, "morton enumeration mismatch");
}

// --------------------------------------------------------------------------------------------
// subdivided_hyper_rectangle + refine_global: bricks in tile-Morton order (gls_box_mesh.hpp), lexicographic nodes
// --------------------------------------------------------------------------------------------
int gls_mesh_hyper_rectangle_sizes(int dim, const int cells[3], int k, int kp, int pmask, int64_t *nc, int64_t *nv,
                                   int64_t *np) {
  if (dim != 3) return set_err(GLS_EINVAL, "gls_mesh_hyper_rectangle: 3D only (dim %d)", dim);
  if (const char *why = gls_impl::box_mesh_sizes(cells, k, kp, pmask, nc, nv, np)) return set_err(GLS_EINVAL, "%s", why);
  return GLS_OK;
}

int gls_mesh_hyper_rectangle(int dim, const int cells[3], int k, int kp, const double p1[3], const double p2[3], int pmask,
                             int32_t *cv, int32_t *cp, double *x0, double *h) {
  if (dim != 3) return set_err(GLS_EINVAL, "gls_mesh_hyper_rectangle: 3D only (dim %d)", dim);
  if (const char *why = gls_impl::box_mesh_fill(cells, k, kp, p1, p2, pmask, cv, cp, x0, h))
    return set_err(GLS_EINVAL, "%s", why);
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// timing
// --------------------------------------------------------------------------------------------
int gls_timing_enable(gls_ctx *c, int en) {
  GLS_TRY(check_ctx(c));
  c->timing = en != 0;
  return GLS_OK;
}
int gls_timing_reset(gls_ctx *c) {
  GLS_TRY(check_ctx(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  c->events.clear();
  for (int i = 0; i < 6; ++i) { c->t_ms[i] = 0; c->t_n[i] = 0; }
  return GLS_OK;
}
int gls_timing_get(gls_ctx *c, int which, double *ms, int64_t *cnt) {
  GLS_TRY(check_ctx(c));
  if (which < 0 || which > 5) return set_err(GLS_EINVAL, "which");
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto &e : c->events) {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e.a, e.b));
    c->t_ms[e.which] += t;
    c->t_n[e.which] += 1;
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  c->events.clear();
  if (ms) *ms = c->t_ms[which];
  if (cnt) *cnt = c->t_n[which];
  return GLS_OK;
}

}  // extern "C"
