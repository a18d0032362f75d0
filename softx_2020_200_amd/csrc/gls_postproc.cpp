// gls_postproc.cpp -- post-processing entry points of the C-ABI: the Kelly error indicator, boundary forces and
// torques, the flow diagnostics (CFL, kinetic energy, enstrophy), the VTU point data evaluated on the device and
// the L2 error against an analytical solution.
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "gls_ctx.hpp"
#include "gls_expr_device.hpp"

using namespace gls_impl;

extern "C" {

// --------------------------------------------------------------------------------------------
// Kelly error indicator (navier_stokes_base.cc:612-652)
// --------------------------------------------------------------------------------------------
namespace {
// face neighbours of a conforming mesh: faces match by their vertex node ids (periodic wraps share
// node ids, so a wrapped face has its periodic neighbour)
int build_face_neighbours(gls_ctx *c) {
  const int dim = c->dim, k = c->k, nv = gls::ipow(k + 1, dim);
  std::vector<int32_t> cn((size_t)c->n_cells * nv);
  if (!cn.empty() && hipMemcpy(cn.data(), c->cell_vnodes.p, cn.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return set_err(GLS_EHIP, "cell map download failed");
  std::map<std::array<int32_t, 4>, std::pair<int, int>> open;  // face key -> (cell, face slot)
  std::vector<int32_t> nbr((size_t)c->n_cells * 2 * dim, -1);
  for (int cell = 0; cell < c->n_cells; ++cell)
    for (int d = 0; d < dim; ++d)
      for (int sd = 0; sd < 2; ++sd) {
        std::array<int32_t, 4> key = {-1, -1, -1, -1};
        int nk = 0;
        for (int v = 0; v < (1 << dim); ++v) {  // cell vertices with coordinate d on side sd
          if (((v >> d) & 1) != sd) continue;
          int a = 0, st = 1;
          for (int e = 0; e < dim; ++e, st *= k + 1) a += ((v >> e) & 1) * k * st;
          key[nk++] = cn[(size_t)cell * nv + a];
        }
        std::sort(key.begin(), key.begin() + nk);
        auto it = open.find(key);
        if (it == open.end()) {
          open.emplace(key, std::make_pair(cell, 2 * d + sd));
        } else {
          nbr[(size_t)cell * 2 * dim + 2 * d + sd] = it->second.first;
          nbr[(size_t)it->second.first * 2 * dim + it->second.second] = cell;
          open.erase(it);
        }
      }
  return c->face_nbr.upload(nbr.data(), nbr.size());
}

gls::KellyTables kelly_tables(int m, int nq) {
  gls::KellyTables T;
  std::memset(&T, 0, sizeof(T));
  double xq[gls::kMaxQ1D], wq[gls::kMaxQ1D], xn[gls::kMaxNodes1D];
  gauss_points(nq, xq, wq);
  lobatto_points(m, xn);
  T.nq = nq;
  for (int a = 0; a <= m; ++a) {
    double v, dd, s2;
    for (int q = 0; q < nq; ++q) {
      lagrange_1d(m, xn, a, xq[q], v, dd, s2);
      T.V[q][a] = v;
    }
    lagrange_1d(m, xn, a, 0.0, v, dd, s2);
    T.De[0][a] = dd;
    lagrange_1d(m, xn, a, 1.0, v, dd, s2);
    T.De[1][a] = dd;
  }
  for (int q = 0; q < nq; ++q) {
    T.w[q] = wq[q];
    T.xq[q] = xq[q];
  }
  for (int a = 0; a <= m; ++a) T.xn[a] = xn[a];
  return T;
}
}  // namespace

int gls_kelly_estimate(gls_ctx *c, const double *sol, int variable, double *eta) {
  GLS_TRY(check_ctx(c));
  if (!sol || !eta || (variable != 0 && variable != 1)) return set_err(GLS_EINVAL, "gls_kelly_estimate: bad arguments");
  if (c->hang.on) return set_err(GLS_EINVAL, "gls_kelly_estimate: conforming meshes only (no hanging nodes)");
  if (c->map_degree > 0) return set_err(GLS_EINVAL, "gls_kelly_estimate: axis-aligned box cells only");
  if (c->nq1d + 1 > gls::kMaxQ1D) return set_err(GLS_EINVAL, "gls_kelly_estimate: face rule too large");
  if (!c->face_nbr.p && c->n_cells > 0) GLS_TRY(build_face_neighbours(c));
  const bool pres = variable == 1;
  const int m = pres ? c->kp : c->k;
  const int32_t *nodes = pres && c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;
  const gls::KellyTables T = kelly_tables(m, c->nq1d + 1);  // QGauss<dim-1>(n_q + 1)
  HIP_TRY(gls::launch_kelly(c->dim, m, nodes, c->face_nbr.p, c->geo.p, sol, c->n_cells, pres ? 1 : c->dim,
                            pres ? (int64_t)c->dim * c->n_vnodes : 0, pres ? 1 : c->dim, T, eta, c->stream));
  return GLS_OK;
}

// Kelly indicator on meshes with hanging faces (gls_octree_faces lists the face pieces): the face
// integrals on the device, then eta_K = sqrt(diam(K)/24 * sum of K's pieces) in a fixed order
int gls_kelly_estimate_faces(gls_ctx *c, const double *sol, int variable, int64_t n_faces, const int32_t *fa,
                             const int32_t *fb, const int32_t *fdir, const double *rect_a, const double *rect_b,
                             double *eta) {
  GLS_TRY(check_ctx(c));
  if (!sol || !eta || (variable != 0 && variable != 1) || n_faces < 0 || (n_faces > 0 && (!fa || !fb || !fdir || !rect_a || !rect_b)))
    return set_err(GLS_EINVAL, "gls_kelly_estimate_faces: bad arguments");
  if (c->map_degree > 0) return set_err(GLS_EINVAL, "gls_kelly_estimate_faces: axis-aligned box cells only");
  for (int64_t e = 0; e < n_faces; ++e)
    if (fa[e] < 0 || fa[e] >= c->n_cells || fb[e] < 0 || fb[e] >= c->n_cells || fdir[e] < 0 || fdir[e] >= c->dim)
      return set_err(GLS_EINVAL, "gls_kelly_estimate_faces: face %lld out of range", (long long)e);
  const bool pres = variable == 1;
  const int m = pres ? c->kp : c->k;
  const int32_t *nodes = pres && c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;
  const gls::KellyTables T = kelly_tables(m, c->nq1d + 1);  // QGauss<dim-1>(n_q + 1) on every piece
  DevBuf<int32_t> dfa, dfb, dfd;
  DevBuf<double> dra, drb, dfi;
  GLS_TRY(dfa.upload(fa, (size_t)n_faces));
  GLS_TRY(dfb.upload(fb, (size_t)n_faces));
  GLS_TRY(dfd.upload(fdir, (size_t)n_faces));
  GLS_TRY(dra.upload(rect_a, (size_t)n_faces * 4));
  GLS_TRY(drb.upload(rect_b, (size_t)n_faces * 4));
  GLS_TRY(dfi.alloc((size_t)std::max<int64_t>(n_faces, 1)));
  HIP_TRY(gls::launch_kelly_faces(c->dim, m, nodes, c->geo.p, sol, n_faces, dfa.p, dfb.p, dfd.p, dra.p, drb.p,
                                  pres ? 1 : c->dim, pres ? (int64_t)c->dim * c->n_vnodes : 0, pres ? 1 : c->dim, T,
                                  dfi.p, c->stream));
  std::vector<double> fi((size_t)n_faces), geo((size_t)c->n_cells * 4), acc((size_t)c->n_cells, 0.0);
  HIP_TRY(hipMemcpyAsync(fi.data(), dfi.p, sizeof(double) * fi.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(geo.data(), c->geo.p, sizeof(double) * geo.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t e = 0; e < n_faces; ++e) {  // each piece counts for both of its cells
    acc[(size_t)fa[e]] += fi[(size_t)e];
    acc[(size_t)fb[e]] += fi[(size_t)e];
  }
  for (int64_t k = 0; k < c->n_cells; ++k) {
    double d2 = 0.0;
    for (int d = 0; d < c->dim; ++d) d2 += geo[(size_t)k * 4 + d] * geo[(size_t)k * 4 + d];
    acc[(size_t)k] = std::sqrt(std::sqrt(d2) / 24.0 * acc[(size_t)k]);
  }
  HIP_TRY(hipMemcpyAsync(eta, acc.data(), sizeof(double) * acc.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

// Kelly indicator on mapped (MappingQ) meshes, conforming or with hanging faces: the face pieces
// and their per-point geometry from gls_fe_space_kelly_faces (host), the jump integrals on the
// device, eta_K = sqrt(diam(K)/24 * sum of K's pieces) in a fixed order (eta: DEVICE pointer)
int gls_kelly_estimate_mapped(gls_ctx *c, const double *sol, int variable, int64_t n_pieces, int nqf, const int32_t *ca,
                              const int32_t *cb, const double *xi, const double *g, const double *jxw,
                              const double *cell_diam, double *eta) {
  GLS_TRY(check_ctx(c));
  if (!sol || !eta || !cell_diam || (variable != 0 && variable != 1) || n_pieces < 0 ||
      (n_pieces > 0 && (!ca || !cb || !xi || !g || !jxw)))
    return set_err(GLS_EINVAL, "gls_kelly_estimate_mapped: bad arguments");
  const int nq = c->nq1d + 1;  // QGauss<dim-1>(n_q + 1)
  if (nqf != (c->dim == 3 ? nq * nq : nq))
    return set_err(GLS_EINVAL, "gls_kelly_estimate_mapped: %d face points per piece, the face rule has %d", nqf,
                   c->dim == 3 ? nq * nq : nq);
  for (int64_t e = 0; e < n_pieces; ++e)
    if (ca[e] < 0 || ca[e] >= c->n_cells || cb[e] < 0 || cb[e] >= c->n_cells)
      return set_err(GLS_EINVAL, "gls_kelly_estimate_mapped: piece %lld out of range", (long long)e);
  const bool pres = variable == 1;
  const int m = pres ? c->kp : c->k;
  const int32_t *nodes = pres && c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;
  const gls::KellyTables T = kelly_tables(m, nq);
  const size_t npts = (size_t)n_pieces * (size_t)nqf;
  DevBuf<int32_t> dca, dcb;
  DevBuf<double> dxi, dg, dj, dfi;
  GLS_TRY(dca.upload(ca, (size_t)n_pieces));
  GLS_TRY(dcb.upload(cb, (size_t)n_pieces));
  GLS_TRY(dxi.upload(xi, npts * 2 * c->dim));
  GLS_TRY(dg.upload(g, npts * 2 * c->dim));
  GLS_TRY(dj.upload(jxw, npts));
  GLS_TRY(dfi.alloc((size_t)std::max<int64_t>(n_pieces, 1)));
  HIP_TRY(gls::launch_kelly_mapped(c->dim, m, nodes, sol, n_pieces, nqf, dca.p, dcb.p, dxi.p, dg.p, dj.p,
                                   pres ? 1 : c->dim, pres ? (int64_t)c->dim * c->n_vnodes : 0, pres ? 1 : c->dim, T,
                                   dfi.p, c->stream));
  std::vector<double> fi((size_t)n_pieces), acc((size_t)c->n_cells, 0.0);
  HIP_TRY(hipMemcpyAsync(fi.data(), dfi.p, sizeof(double) * fi.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t e = 0; e < n_pieces; ++e) {  // each piece counts for both of its cells
    acc[(size_t)ca[e]] += fi[(size_t)e];
    acc[(size_t)cb[e]] += fi[(size_t)e];
  }
  for (int64_t k = 0; k < c->n_cells; ++k) acc[(size_t)k] = std::sqrt(cell_diam[k] / 24.0 * acc[(size_t)k]);
  HIP_TRY(hipMemcpyAsync(eta, acc.data(), sizeof(double) * acc.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// Forces and torques on the boundaries (postprocessing_force.cc, postprocessing_torque.cc): the face
// data of one mesh uploaded once (plan), every evaluation one pass over all boundaries on the device
// --------------------------------------------------------------------------------------------
struct gls_boundary_plan {
  gls_ctx *ctx = nullptr;
  int64_t n_faces = 0, n_pts = 0;
  int nqf = 0, n_slots = 0;
  DevBuf<int32_t> cell, slot;
  DevBuf<double> xi, jinv, normal, jxw, xq, cor, partial, out;
};

namespace {
int boundary_degrees(gls_ctx *c, const char *who) {
  if (!gls::boundary_loads_supported(c->dim, c->k, c->kp))
    return set_err(GLS_EINVAL,
                   "%s: FE_Q(%d)-FE_Q(%d) in %dD has no load kernel (velocity / pressure orders (1,1), (2,1), (2,2); "
                   "2D Q3 is not supported)",
                   who, c->k, c->kp, c->dim);
  return GLS_OK;
}
}  // namespace

int gls_boundary_plan_create(gls_ctx *c, int64_t n_faces, int nqf, const int32_t *cell, const int32_t *slot,
                             const double *xi, const double *jinv, const double *normal, const double *jxw,
                             const double *xq, int n_slots, gls_boundary_plan **out) {
  GLS_TRY(check_ctx(c));
  if (!out || n_faces < 0 || nqf < 1 || n_slots < 1 || n_slots > 4096 ||
      (n_faces > 0 && (!cell || !slot || !xi || !jinv || !normal || !jxw || !xq)))
    return set_err(GLS_EINVAL, "gls_boundary_plan_create: bad arguments");
  GLS_TRY(boundary_degrees(c, "gls_boundary_plan_create"));
  for (int64_t f = 0; f < n_faces; ++f)
    if (cell[f] < 0 || cell[f] >= c->n_cells || slot[f] < -1 || slot[f] >= n_slots)
      return set_err(GLS_EINVAL, "gls_boundary_plan_create: face %lld: cell %d / slot %d out of range", (long long)f,
                     cell[f], slot[f]);
  std::unique_ptr<gls_boundary_plan> p(new gls_boundary_plan);
  p->ctx = c;
  p->n_faces = n_faces;
  p->nqf = nqf;
  p->n_slots = n_slots;
  p->n_pts = n_faces * nqf;
  const size_t np = (size_t)p->n_pts, dim = (size_t)c->dim;
  GLS_TRY(p->cell.upload(cell, (size_t)n_faces));
  GLS_TRY(p->slot.upload(slot, (size_t)n_faces));
  GLS_TRY(p->xi.upload(xi, np * dim));
  GLS_TRY(p->jinv.upload(jinv, np * dim * dim));
  GLS_TRY(p->normal.upload(normal, np * dim));
  GLS_TRY(p->jxw.upload(jxw, np));
  GLS_TRY(p->xq.upload(xq, np * dim));
  GLS_TRY(p->cor.alloc((size_t)n_slots * 3));
  GLS_TRY(p->partial.alloc((size_t)std::max<int64_t>(gls::boundary_loads_blocks(p->n_pts), 1) * n_slots * 6));
  GLS_TRY(p->out.alloc((size_t)n_slots * 6));
  *out = p.release();
  return GLS_OK;
}

int gls_boundary_plan_destroy(gls_boundary_plan *plan) {
  delete plan;
  return GLS_OK;
}

int gls_boundary_loads(gls_ctx *c, gls_boundary_plan *p, const double *sol, double viscosity, const double *cor,
                       double *force, double *torque) {
  GLS_TRY(check_ctx(c));
  if (!p || p->ctx != c) return set_err(GLS_EINVAL, "gls_boundary_loads: the plan belongs to another context");
  if (!sol || !cor || !force || !torque) return set_err(GLS_EINVAL, "gls_boundary_loads: bad arguments");
  GLS_TRY(boundary_degrees(c, "gls_boundary_loads"));
  const int ns = p->n_slots;
  std::fill(force, force + 3 * ns, 0.0);
  std::fill(torque, torque + 3 * ns, 0.0);
  if (p->n_pts == 0) return GLS_OK;
  HIP_TRY(hipMemcpyAsync(p->cor.p, cor, sizeof(double) * 3 * (size_t)ns, hipMemcpyHostToDevice, c->stream));
  const int32_t *pn = c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;  // equal order: shared nodes
  HIP_TRY(gls::launch_boundary_loads(c->dim, c->k, c->kp, c->cell_vnodes.p, pn, sol, (int64_t)c->dim * c->n_vnodes,
                                     p->n_pts, p->nqf, p->cell.p, p->slot.p, p->xi.p, p->jinv.p, p->normal.p, p->jxw.p,
                                     p->xq.p, viscosity, p->cor.p, ns, p->partial.p, p->out.p, c->stream));
  std::vector<double> o((size_t)ns * 6);
  HIP_TRY(hipMemcpyAsync(o.data(), p->out.p, sizeof(double) * o.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int s = 0; s < ns; ++s)
    for (int i = 0; i < 3; ++i) {
      force[3 * s + i] = o[(size_t)(6 * s + i)];
      torque[3 * s + i] = o[(size_t)(6 * s + 3 + i)];
    }
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// Flow diagnostics (postprocessing_cfl.cc, postprocessing_kinetic_energy.cc, postprocessing_enstrophy.cc):
// one pass over the context's cells, per-block partials and one ordered stage on the device
// --------------------------------------------------------------------------------------------
int gls_flow_diagnostics(gls_ctx *c, const double *sol, double dt, double out[4]) {
  GLS_TRY(check_ctx(c));
  if (!sol || !out) return set_err(GLS_EINVAL, "gls_flow_diagnostics: bad arguments");
  if (!gls::flow_diagnostics_supported(c->dim, c->k, c->kp) || c->nq1d != c->k + 1)
    return set_err(GLS_EINVAL,
                   "gls_flow_diagnostics: FE_Q(%d)-FE_Q(%d) in %dD with QGauss(%d) has no diagnostics kernel (velocity / "
                   "pressure orders (1,1), (2,1), (2,2) with QGauss(k+1); 2D Q3 is not supported)",
                   c->k, c->kp, c->dim, c->nq1d);
  for (int i = 0; i < 4; ++i) out[i] = 0.0;
  if (c->n_cells == 0) return GLS_OK;
  if (!c->fd_out.p) {  // once per context: cell measures, 1D tables, partials
    const int dim = c->dim, k1 = c->k + 1;
    std::vector<double> meas((size_t)c->n_cells, 1.0);
    if (c->map_degree > 0) {
      const size_t nsup = (size_t)gls::ipow(c->map_degree + 1, dim);
      for (int cix = 0; cix < c->n_cells; ++cix)
        meas[(size_t)cix] = corner_measure(dim, c->map_degree, c->host_support.data() + (size_t)cix * nsup * dim);
    } else {
      for (int cix = 0; cix < c->n_cells; ++cix)
        for (int e = 0; e < dim; ++e) meas[(size_t)cix] *= c->host_h[(size_t)cix * dim + e];
    }
    std::vector<double> tab((size_t)(2 * k1 * k1 + k1));
    for (int q = 0; q < k1; ++q) {
      for (int a = 0; a < k1; ++a) {
        tab[(size_t)(q * k1 + a)] = c->tables.V[q][a];
        tab[(size_t)(k1 * k1 + q * k1 + a)] = c->tables.D[q][a];
      }
      tab[(size_t)(2 * k1 * k1 + q)] = c->tables.w[q];
    }
    GLS_TRY(c->fd_meas.upload(meas.data(), meas.size()));
    GLS_TRY(c->fd_tab.upload(tab.data(), tab.size()));
    GLS_TRY(c->fd_partial.alloc((size_t)gls::flow_diagnostics_blocks(c->n_cells) * 4));
    GLS_TRY(c->fd_out.alloc(4));
  }
  HIP_TRY(gls::launch_flow_diagnostics(c->dim, c->k, c->cell_vnodes.p, c->geo.p, c->gq.p, c->fd_meas.p, c->fd_tab.p, sol,
                                       c->n_cells, dt, c->fd_partial.p, c->fd_out.p, c->stream));
  HIP_TRY(hipMemcpyAsync(out, c->fd_out.p, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

// --------------------------------------------------------------------------------------------
// VTU point data on the device (navier_stokes_base.cc:1035-1064, post_processors.h:27-171): the geometry of
// one mesh and the 1D tables at the patch points uploaded once (plan), every output one launch over all
// cells, one download per array and the file writer of gls_vtu_write
// --------------------------------------------------------------------------------------------
}  // extern "C"
// gls_io.cpp: the 1D tables and the file writer shared with gls_vtu_write
void gls_io_patch_tables(int degree, int ns, double *V, double *D);
int gls_io_vtu_write_piece(const char *filename, int dim, int k, int64_t nc, int ns, int subdomain, int binary, int srf,
                           const double *pts, const double *vel, const double *pre, const double *vort,
                           const double *qcr, const double *eul, double *encode_seconds);
extern "C" {

struct gls_output_plan {
  gls_ctx *ctx = nullptr;
  int ns = 1, srf = 0;
  double omega[3] = {0, 0, 0};
  int64_t n_pts = 0;
  DevBuf<double> x0h, support, tab;
  DevBuf<double> pts, vel, pre, vort, qcr, eul;  // the device field buffers, allocated once
  std::vector<double> h_pts, h_vel, h_pre, h_vort, h_qcr, h_eul;  // gls_vtu_write_device: the downloaded arrays
};

int gls_output_plan_create(gls_ctx *c, const gls_mesh_desc *m, int subdivision, gls_output_plan **out) {
  GLS_TRY(check_ctx(c));
  if (!m || !out) return set_err(GLS_EINVAL, "gls_output_plan_create: null argument");
  if (m->dim != c->dim || m->k != c->k || m->kp != c->kp || m->n_cells != c->n_cells || m->map_degree != c->map_degree)
    return set_err(GLS_EINVAL,
                   "gls_output_plan_create: the mesh (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d) is not the "
                   "context's (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d)",
                   m->dim, m->k, m->kp, m->n_cells, m->map_degree, c->dim, c->k, c->kp, c->n_cells, c->map_degree);
  if (!gls::output_fields_supported(c->dim, c->k, c->kp, c->map_degree, subdivision))
    return set_err(GLS_EINVAL,
                   "gls_output_plan_create: FE_Q(%d)-FE_Q(%d) in %dD with subdivision %d has no output kernel (velocity / "
                   "pressure orders (1,1), (2,1), (2,2), 2D Q3 is not supported; (subdivision+1)^dim <= 256: subdivision "
                   "1..15 in 2D, 1..5 in 3D)",
                   c->k, c->kp, c->dim, subdivision);
  const int dim = c->dim, md = c->map_degree, np1 = subdivision + 1;
  if (md ? !m->cell_support : !m->cell_h)
    return set_err(GLS_EINVAL, "gls_output_plan_create: the mesh has no %s", md ? "cell_support" : "cell_h");
  std::unique_ptr<gls_output_plan> p(new gls_output_plan);
  p->ctx = c;
  p->ns = subdivision;
  p->srf = m->srf ? 1 : 0;
  for (int i = 0; i < 3; ++i) p->omega[i] = m->omega[i];
  const size_t nc = (size_t)c->n_cells;
  p->n_pts = (int64_t)nc * gls::ipow(np1, dim);
  if (md) {
    GLS_TRY(p->support.upload(m->cell_support, nc * (size_t)gls::ipow(md + 1, dim) * dim));
  } else {
    std::vector<double> x0h(nc * 2 * dim);
    for (size_t cix = 0; cix < nc; ++cix)
      for (int d = 0; d < dim; ++d) {
        x0h[cix * 2 * dim + d] = m->cell_x0 ? m->cell_x0[cix * dim + d] : 0.0;
        x0h[cix * 2 * dim + dim + d] = m->cell_h[cix * dim + d];
      }
    GLS_TRY(p->x0h.upload(x0h.data(), x0h.size()));
  }
  // Vv | Dv | Vp | Vm | Dm at t / subdivision
  const int k1 = c->k + 1, kp1 = c->kp + 1, nm = md ? md + 1 : 0;
  std::vector<double> tab((size_t)np1 * (2 * k1 + kp1 + 2 * nm));
  gls_io_patch_tables(c->k, subdivision, tab.data(), tab.data() + np1 * k1);
  gls_io_patch_tables(c->kp, subdivision, tab.data() + 2 * np1 * k1, nullptr);  // the pressure enters by value only
  if (md) gls_io_patch_tables(md, subdivision, tab.data() + np1 * (2 * k1 + kp1), tab.data() + np1 * (2 * k1 + kp1 + nm));
  GLS_TRY(p->tab.upload(tab.data(), tab.size()));
  const size_t np = (size_t)p->n_pts;
  GLS_TRY(p->pts.alloc(np * 3));
  GLS_TRY(p->vel.alloc(np * 3));
  GLS_TRY(p->pre.alloc(np));
  GLS_TRY(p->vort.alloc(np * (dim == 3 ? 3 : 1)));
  GLS_TRY(p->qcr.alloc(np));
  if (p->srf) GLS_TRY(p->eul.alloc(np * 3));
  *out = p.release();
  return GLS_OK;
}

int gls_output_plan_destroy(gls_output_plan *plan) {
  delete plan;
  return GLS_OK;
}

namespace {
// the launch and one download per array, all on the context's stream; the caller synchronizes
int output_fields_queue(gls_ctx *c, gls_output_plan *p, const double *sol, double *pts, double *vel, double *pre,
                        double *vort, double *qcr, double *eul) {
  const size_t np = (size_t)p->n_pts;
  if (np == 0) return GLS_OK;
  if (!c->cell_pnodes.p && c->kp != c->k) return set_err(GLS_EINVAL, "output fields: the context has no cell_pnodes");
  const int32_t *pn = c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;  // equal order: shared nodes
  HIP_TRY(gls::launch_output_fields(c->dim, c->k, c->kp, c->map_degree, p->ns, c->cell_vnodes.p, pn, sol,
                                    (int64_t)c->dim * c->n_vnodes, p->x0h.p, p->support.p, p->tab.p, c->n_cells, p->srf,
                                    p->omega, p->pts.p, p->vel.p, p->pre.p, p->vort.p, p->qcr.p, p->eul.p, c->stream));
  const struct { double *h; const double *d; size_t n; } a[6] = {
      {pts, p->pts.p, np * 3}, {vel, p->vel.p, np * 3}, {pre, p->pre.p, np}, {vort, p->vort.p, np * (c->dim == 3 ? 3 : 1)},
      {qcr, p->qcr.p, np},     {p->srf ? eul : nullptr, p->eul.p, np * 3}};
  for (const auto &x : a)
    if (x.h) HIP_TRY(hipMemcpyAsync(x.h, x.d, sizeof(double) * x.n, hipMemcpyDeviceToHost, c->stream));
  return GLS_OK;
}
int output_plan_check(gls_ctx *c, gls_output_plan *p, const double *sol, const char *who) {
  GLS_TRY(check_ctx(c));
  if (!p || p->ctx != c) return set_err(GLS_EINVAL, "%s: the plan belongs to another context", who);
  if (!sol) return set_err(GLS_EINVAL, "%s: null solution", who);
  if (p->n_pts != (int64_t)c->n_cells * gls::ipow(p->ns + 1, c->dim))
    return set_err(GLS_EINVAL, "%s: the context has changed since the plan was made", who);
  return GLS_OK;
}
}  // namespace

int gls_output_fields(gls_ctx *c, gls_output_plan *p, const double *sol, double *points, double *velocity,
                      double *pressure, double *vorticity, double *q_criterion, double *velocity_eulerian) {
  GLS_TRY(output_plan_check(c, p, sol, "gls_output_fields"));
  if (!points || !velocity || !pressure || !vorticity || !q_criterion || (p->srf && !velocity_eulerian))
    return set_err(GLS_EINVAL, "gls_output_fields: null output array");
  GLS_TRY(output_fields_queue(c, p, sol, points, velocity, pressure, vorticity, q_criterion, velocity_eulerian));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

int gls_vtu_write_device(gls_ctx *c, gls_output_plan *p, const double *sol, const char *filename, int subdomain,
                         int binary) {
  GLS_TRY(output_plan_check(c, p, sol, "gls_vtu_write_device"));
  if (!filename) return set_err(GLS_EINVAL, "gls_vtu_write_device: null file name");
  // GLS_OUTPUT_SPLIT=1: host clocks to the synchronization, around the encoding and over the writer, on stderr
  static const bool split = std::getenv("GLS_OUTPUT_SPLIT") != nullptr;
  double enc = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t np = (size_t)p->n_pts;
  if (p->h_pts.size() != np * 3) {  // once per plan
    p->h_pts.resize(np * 3);
    p->h_vel.resize(np * 3);
    p->h_pre.resize(np);
    p->h_vort.resize(np * (c->dim == 3 ? 3 : 1));
    p->h_qcr.resize(np);
    if (p->srf) p->h_eul.resize(np * 3);
  }
  GLS_TRY(output_fields_queue(c, p, sol, p->h_pts.data(), p->h_vel.data(), p->h_pre.data(), p->h_vort.data(),
                              p->h_qcr.data(), p->h_eul.data()));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const auto t1 = std::chrono::steady_clock::now();
  const int rc = gls_io_vtu_write_piece(filename, c->dim, c->k, c->n_cells, p->ns, subdomain, binary, p->srf,
                                        p->h_pts.data(), p->h_vel.data(), p->h_pre.data(), p->h_vort.data(),
                                        p->h_qcr.data(), p->srf ? p->h_eul.data() : nullptr, split ? &enc : nullptr);
  if (split) {
    const double dl = std::chrono::duration<double>(t1 - t0).count();
    const double wr = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    std::fprintf(stderr, "gls_vtu_write_device: launch + downloads %.6f s, encode %.6f s, file write %.6f s\n", dl, enc,
                 wr - enc);
  }
  return rc;
}

// --------------------------------------------------------------------------------------------
// L2 error against an analytical solution (the application's l2_error(), the reference's calculate_L2_error):
// the geometry of one mesh and the 1D tables at the QGauss(k+2) abscissae uploaded once (plan), every evaluation
// two passes over all cells on the device and one download of the sums
// --------------------------------------------------------------------------------------------
struct gls_error_plan {
  gls_ctx *ctx = nullptr;
  gls::expr::DeviceProgram exact;
  int64_t n_cells = 0;
  double volume = -1.0;  // general meshes: the sum of the Q1 cell measures; boxes: < 0, the sum of JxW
  DevBuf<double> x0h, support, tab, partial, out;
};

int gls_error_plan_create(gls_ctx *c, const gls_mesh_desc *m, const gls_expr *exact, gls_error_plan **out) {
  GLS_TRY(check_ctx(c));
  if (!m || !exact || !out) return set_err(GLS_EINVAL, "gls_error_plan_create: null argument");
  if (c->dist.on) return set_err(GLS_EINVAL, "gls_error_plan_create: a distributed context is not served");
  if (m->dim != c->dim || m->k != c->k || m->kp != c->kp || m->n_cells != c->n_cells || m->map_degree != c->map_degree)
    return set_err(GLS_EINVAL,
                   "gls_error_plan_create: the mesh (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d) is not the "
                   "context's (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d)",
                   m->dim, m->k, m->kp, m->n_cells, m->map_degree, c->dim, c->k, c->kp, c->n_cells, c->map_degree);
  const int dim = c->dim, md = c->map_degree, k1 = c->k + 1, kp1 = c->kp + 1, nq1 = c->k + 2, nm = md ? md + 1 : 0;
  if (!gls::l2_error_supported(dim, c->k, c->kp, md, 1))
    return set_err(GLS_EINVAL,
                   "gls_error_plan_create: FE_Q(%d)-FE_Q(%d) in %dD with mapping degree %d has no L2 error kernel "
                   "(velocity / pressure orders (1,1), (2,1), (2,2), 2D Q3 is not supported; mapping degree <= 3)",
                   c->k, c->kp, dim, md);
  std::unique_ptr<gls_error_plan> p(new gls_error_plan);
  GLS_TRY(gls::expr::device_program(exact, "gls_error_plan_create", &p->exact));  // GLS_EINVAL: stack past the cap
  if (p->exact.n_vars != dim + 1)
    return set_err(GLS_EINVAL, "gls_error_plan_create: the analytical solution has %d variables, expected %d (%s, t)",
                   p->exact.n_vars, dim + 1, dim == 3 ? "x, y, z" : "x, y");
  if (p->exact.n_comps < dim)
    return set_err(GLS_EINVAL,
                   "gls_error_plan_create: the analytical solution has %d components, expected the %d velocity "
                   "components and optionally the pressure",
                   p->exact.n_comps, dim);
  if (!gls::l2_error_supported(dim, c->k, c->kp, md, p->exact.max_stack))
    return set_err(GLS_EINVAL, "gls_error_plan_create: no launch shape for an operand stack of %d entries",
                   p->exact.max_stack);
  if (md ? !m->cell_support : !m->cell_h)
    return set_err(GLS_EINVAL, "gls_error_plan_create: the mesh has no %s", md ? "cell_support" : "cell_h");
  if (!c->cell_pnodes.p && c->kp != c->k) return set_err(GLS_EINVAL, "gls_error_plan_create: the context has no cell_pnodes");
  p->ctx = c;
  const size_t nc = (size_t)c->n_cells;
  p->n_cells = c->n_cells;
  if (md) {
    const size_t nsup = (size_t)gls::ipow(md + 1, dim);
    GLS_TRY(p->support.upload(m->cell_support, nc * nsup * dim));
    p->volume = 0.0;  // GridTools::volume: the cells' Q1 measures, summed in cell order
    for (size_t cix = 0; cix < nc; ++cix) p->volume += corner_measure(dim, md, m->cell_support + cix * nsup * dim);
  } else {
    std::vector<double> x0h(nc * 2 * dim);
    for (size_t cix = 0; cix < nc; ++cix)
      for (int d = 0; d < dim; ++d) {
        x0h[cix * 2 * dim + d] = m->cell_x0 ? m->cell_x0[cix * dim + d] : 0.0;
        x0h[cix * 2 * dim + dim + d] = m->cell_h[cix * dim + d];
      }
    GLS_TRY(p->x0h.upload(x0h.data(), x0h.size()));
  }
  // Vv | Vp | xq | wq | Vm | Dm at the QGauss(k+2) abscissae
  std::vector<double> tab((size_t)nq1 * (k1 + kp1 + 2 + 2 * nm)), xq((size_t)nq1), wq((size_t)nq1);
  gauss_points(nq1, xq.data(), wq.data());
  double *tVv = tab.data(), *tVp = tVv + nq1 * k1, *tX = tVp + nq1 * kp1, *tW = tX + nq1, *tVm = tW + nq1,
         *tDm = tVm + nq1 * nm;
  double xn[gls::kMaxNodes1D], dv, ddv;
  for (int q = 0; q < nq1; ++q) {
    tX[q] = xq[(size_t)q];
    tW[q] = wq[(size_t)q];
    lobatto_points(c->k, xn);
    for (int a = 0; a < k1; ++a) lagrange_1d(c->k, xn, a, xq[(size_t)q], tVv[q * k1 + a], dv, ddv);
    lobatto_points(c->kp, xn);
    for (int a = 0; a < kp1; ++a) lagrange_1d(c->kp, xn, a, xq[(size_t)q], tVp[q * kp1 + a], dv, ddv);
    if (md) {
      lobatto_points(md, xn);
      for (int a = 0; a < nm; ++a) lagrange_1d(md, xn, a, xq[(size_t)q], tVm[q * nm + a], tDm[q * nm + a], ddv);
    }
  }
  GLS_TRY(p->tab.upload(tab.data(), tab.size()));
  GLS_TRY(p->partial.alloc((size_t)gls::l2_error_blocks(dim, c->k, c->kp, md, p->exact.max_stack, c->n_cells) * 3));
  GLS_TRY(p->out.alloc(6));
  *out = p.release();
  return GLS_OK;
}

int gls_error_plan_destroy(gls_error_plan *plan) {
  delete plan;
  return GLS_OK;
}

int gls_l2_error(gls_ctx *c, gls_error_plan *p, const double *sol, double time, double out[2]) {
  GLS_TRY(check_ctx(c));
  if (!p || p->ctx != c) return set_err(GLS_EINVAL, "gls_l2_error: the plan belongs to another context");
  if (!sol || !out) return set_err(GLS_EINVAL, "gls_l2_error: bad arguments");
  if (p->n_cells != c->n_cells) return set_err(GLS_EINVAL, "gls_l2_error: the context has changed since the plan was made");
  out[0] = out[1] = 0.0;
  if (c->n_cells == 0) return GLS_OK;
  const int32_t *pn = c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;  // equal order: shared nodes
  HIP_TRY(gls::launch_l2_error(c->dim, c->k, c->kp, c->map_degree, c->cell_vnodes.p, pn, sol,
                               (int64_t)c->dim * c->n_vnodes, p->x0h.p, p->support.p, p->tab.p, c->n_cells, p->exact, time,
                               p->volume, p->partial.p, p->out.p, c->stream));
  double h[6];
  HIP_TRY(hipMemcpyAsync(h, p->out.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  out[0] = std::sqrt(h[3]);
  out[1] = std::sqrt(h[4]);
  return GLS_OK;
}

}  // extern "C"
