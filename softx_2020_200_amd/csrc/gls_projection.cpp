// gls_projection.cpp -- the L2-projection initial condition on the device (the reference's assemble_L2_projection +
// solve_system_GMRES(.., 1e-15, 1e-15), gls_navier_stokes.cc:795-803, 830-914; the application's host
// l2_projection()): the matrix-free consistent mass operator of gls_mass.hip, its right-hand side from an
// expression's bytecode, and Jacobi-preconditioned conjugate gradients in FP64 on the context's stream.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "gls_ctx.hpp"
#include "gls_expr_device.hpp"
#include "gls_incidence.hpp"

using namespace gls_impl;

extern "C" {

struct gls_projection_plan {
  gls_ctx *ctx = nullptr;
  int64_t n_cells = 0, n_dofs = 0;
  DevBuf<double> x0h, support, tab;
  DevBuf<double> ev;                          // element vectors [n_cells][NV dim + NP]
  DevBuf<int64_t> voff, vslot, poff, pslot;   // node -> slots of ev, ascending in cell
  DevBuf<double> diag;                        // the mass diagonal, no constraint mask
  DevBuf<double> vec;                         // CG: b | r | z | p | M p | diagonal with 1 on the Dirichlet rows
  DevBuf<double> scal;                        // the dots on the device
};

namespace {

constexpr int kProjectionMaxIterations = 10000;
constexpr double kProjectionTolerance = 1e-15;  // relative residual

// y = per-node sums of the plan's element vectors
int mass_gather(gls_ctx *c, gls_projection_plan *p, double *y) {
  HIP_TRY(gls::gather_element_vectors(y, p->ev.p, p->voff.p, p->vslot.p, c->n_vnodes, p->poff.p, p->pslot.p,
                                      c->n_pnodes, c->dim, c->stream));
  return GLS_OK;
}

int mass_launch(gls_ctx *c, gls_projection_plan *p, int mode, const double *x, const gls::expr::DeviceProgram *f,
                double time) {
  const int32_t *pn = c->cell_pnodes.p ? c->cell_pnodes.p : c->cell_vnodes.p;  // equal order: shared nodes
  HIP_TRY(gls::launch_mass(mode, c->dim, c->k, c->kp, c->map_degree, c->cell_vnodes.p, pn, x,
                           (int64_t)c->dim * c->n_vnodes, p->x0h.p, p->support.p, p->tab.p, c->n_cells, f, time, p->ev.p,
                           c->stream));
  return GLS_OK;
}

// y = M x; masked: the rows of the context's Dirichlet set zeroed (P M P on vectors that vanish there)
int mass_apply(gls_ctx *c, gls_projection_plan *p, const double *x, double *y, bool masked) {
  GLS_TRY(mass_launch(c, p, gls::kMassApply, x, nullptr, 0.0));
  GLS_TRY(mass_gather(c, p, y));
  if (masked && c->dir_dofs.n)
    HIP_TRY(gls::vec_set_indexed(y, c->dir_dofs.p, nullptr, (int64_t)c->dir_dofs.n, c->stream));
  return GLS_OK;
}

// out[i] = a_i . w for nk vectors a_0, a_1 = a_0 + lda, ... (HOST result: one read-back)
int dots(gls_ctx *c, gls_projection_plan *p, const double *a, int64_t lda, int nk, const double *w, double *out) {
  HIP_TRY(gls::vec_multidot(a, lda, nk, w, p->n_dofs, p->scal.p, c->work.p, c->stream));
  HIP_TRY(hipMemcpyAsync(out, p->scal.p, sizeof(double) * (size_t)nk, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GLS_OK;
}

int plan_check(gls_ctx *c, gls_projection_plan *p, const char *who) {
  GLS_TRY(check_ctx(c));
  if (!p || p->ctx != c) return set_err(GLS_EINVAL, "%s: the plan belongs to another context", who);
  if (p->n_cells != c->n_cells || p->n_dofs != c->n_dofs)
    return set_err(GLS_EINVAL, "%s: the context has changed since the plan was made", who);
  if (c->hang.on) return set_err(GLS_EINVAL, "%s: the context has hanging or slip lines (gls_set_hanging)", who);
  return GLS_OK;
}

}  // namespace

int gls_projection_plan_create(gls_ctx *c, const gls_mesh_desc *m, gls_projection_plan **out) {
  GLS_TRY(check_ctx(c));
  if (!m || !out) return set_err(GLS_EINVAL, "gls_projection_plan_create: null argument");
  if (c->dist.on) return set_err(GLS_EINVAL, "gls_projection_plan_create: a distributed context is not served");
  if (m->dim != c->dim || m->k != c->k || m->kp != c->kp || m->n_cells != c->n_cells || m->map_degree != c->map_degree)
    return set_err(GLS_EINVAL,
                   "gls_projection_plan_create: the mesh (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d) is not the "
                   "context's (%dD FE_Q(%d)-FE_Q(%d), %d cells, mapping degree %d)",
                   m->dim, m->k, m->kp, m->n_cells, m->map_degree, c->dim, c->k, c->kp, c->n_cells, c->map_degree);
  const int dim = c->dim, md = c->map_degree, k1 = c->k + 1, kp1 = c->kp + 1, nq1 = c->k + 1, nm = md ? md + 1 : 0;
  if (!gls::mass_supported(dim, c->k, c->kp, md, 0))
    return set_err(GLS_EINVAL,
                   "gls_projection_plan_create: FE_Q(%d)-FE_Q(%d) in %dD with mapping degree %d has no mass kernel "
                   "(velocity / pressure orders (1,1), (2,1), (2,2), 2D Q3 is not supported; mapping degree <= 3)",
                   c->k, c->kp, dim, md);
  if (c->hang.on)
    return set_err(GLS_EINVAL,
                   "gls_projection_plan_create: the context has hanging or slip lines (gls_set_hanging); the projection "
                   "holds only the Dirichlet set of gls_set_dirichlet fixed");
  if (md ? !m->cell_support : !m->cell_h)
    return set_err(GLS_EINVAL, "gls_projection_plan_create: the mesh has no %s", md ? "cell_support" : "cell_h");
  if (!c->cell_pnodes.p && c->kp != c->k)
    return set_err(GLS_EINVAL, "gls_projection_plan_create: the context has no cell_pnodes");
  std::unique_ptr<gls_projection_plan> p(new gls_projection_plan);
  p->ctx = c;
  p->n_cells = c->n_cells;
  p->n_dofs = c->n_dofs;
  const size_t nc = (size_t)c->n_cells, n = (size_t)c->n_dofs;
  GLS_TRY(p->scal.alloc(2));
  GLS_TRY(p->diag.alloc(std::max<size_t>(n, 1)));
  if (nc == 0) {
    HIP_TRY(gls::vec_fill(p->diag.p, (int64_t)n, 0.0, c->stream));
    *out = p.release();
    return GLS_OK;
  }
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
  // Vv | Vp | xq | wq | Vv^2 | Vp^2 | Vm | Dm at the QGauss(k+1) abscissae
  std::vector<double> tab((size_t)nq1 * (2 * k1 + 2 * kp1 + 2 + 2 * nm)), xq((size_t)nq1), wq((size_t)nq1);
  gauss_points(nq1, xq.data(), wq.data());
  double *tVv = tab.data(), *tVp = tVv + nq1 * k1, *tX = tVp + nq1 * kp1, *tW = tX + nq1, *tVv2 = tW + nq1,
         *tVp2 = tVv2 + nq1 * k1, *tVm = tVp2 + nq1 * kp1, *tDm = tVm + nq1 * nm;
  double xn[gls::kMaxNodes1D], dv, ddv;
  for (int q = 0; q < nq1; ++q) {
    tX[q] = xq[(size_t)q];
    tW[q] = wq[(size_t)q];
    lobatto_points(c->k, xn);
    for (int a = 0; a < k1; ++a) {
      lagrange_1d(c->k, xn, a, xq[(size_t)q], tVv[q * k1 + a], dv, ddv);
      tVv2[q * k1 + a] = tVv[q * k1 + a] * tVv[q * k1 + a];
    }
    lobatto_points(c->kp, xn);
    for (int a = 0; a < kp1; ++a) {
      lagrange_1d(c->kp, xn, a, xq[(size_t)q], tVp[q * kp1 + a], dv, ddv);
      tVp2[q * kp1 + a] = tVp[q * kp1 + a] * tVp[q * kp1 + a];
    }
    if (md) {
      lobatto_points(md, xn);
      for (int a = 0; a < nm; ++a) lagrange_1d(md, xn, a, xq[(size_t)q], tVm[q * nm + a], tDm[q * nm + a], ddv);
    }
  }
  GLS_TRY(p->tab.upload(tab.data(), tab.size()));
  // node -> (cell, slot), ascending in cell: the fixed order of the node sums
  const int nv = gls::ipow(k1, dim), np = gls::ipow(kp1, dim);
  std::vector<int32_t> cv(nc * nv), cp;
  HIP_TRY(hipMemcpy(cv.data(), c->cell_vnodes.p, cv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (c->cell_pnodes.p) {
    cp.resize(nc * np);
    HIP_TRY(hipMemcpy(cp.data(), c->cell_pnodes.p, cp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  ElementIncidence I;
  if (!element_incidence(c->n_cells, dim, nv, np, c->n_vnodes, c->n_pnodes, cv.data(),
                         c->cell_pnodes.p ? cp.data() : cv.data(), I))
    return set_err(GLS_EINVAL, "gls_projection_plan_create: a cell's node id is out of range");
  GLS_TRY(p->voff.upload(I.voff.data(), I.voff.size()));
  GLS_TRY(p->vslot.upload(I.vslot.data(), I.vslot.size()));
  GLS_TRY(p->poff.upload(I.poff.data(), I.poff.size()));
  GLS_TRY(p->pslot.upload(I.pslot.data(), I.pslot.size()));
  GLS_TRY(p->ev.alloc(nc * ((size_t)nv * dim + np)));
  // the diagonal: one launch
  GLS_TRY(mass_launch(c, p.get(), gls::kMassDiag, nullptr, nullptr, 0.0));
  GLS_TRY(mass_gather(c, p.get(), p->diag.p));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = p.release();
  return GLS_OK;
}

int gls_projection_plan_destroy(gls_projection_plan *plan) {
  delete plan;
  return GLS_OK;
}

int gls_mass_apply(gls_ctx *c, gls_projection_plan *p, const double *x, double *y) {
  GLS_TRY(plan_check(c, p, "gls_mass_apply"));
  if (!x || !y || x == y) return set_err(GLS_EINVAL, "gls_mass_apply: x / y null or aliased");
  if (c->n_cells == 0) {
    HIP_TRY(gls::vec_fill(y, c->n_dofs, 0.0, c->stream));
    return GLS_OK;
  }
  return mass_apply(c, p, x, y, false);
}

int gls_mass_diagonal(gls_ctx *c, gls_projection_plan *p, double *d) {
  GLS_TRY(plan_check(c, p, "gls_mass_diagonal"));
  if (!d) return set_err(GLS_EINVAL, "gls_mass_diagonal: null argument");
  HIP_TRY(gls::vec_copy(d, p->diag.p, c->n_dofs, c->stream));
  return GLS_OK;
}

int gls_l2_projection(gls_ctx *c, gls_projection_plan *p, const gls_expr *f, double time, double *x,
                      gls_projection_info *info) {
  GLS_TRY(plan_check(c, p, "gls_l2_projection"));
  if (!f || !x) return set_err(GLS_EINVAL, "gls_l2_projection: null argument");
  if (info) {
    info->iterations = 0;
    info->relative_residual = 0.0;
  }
  const int dim = c->dim;
  gls::expr::DeviceProgram prog;
  GLS_TRY(gls::expr::device_program(f, "gls_l2_projection", &prog));  // GLS_EINVAL: stack past the cap
  if (prog.n_comps != dim + 1)
    return set_err(GLS_EINVAL, "gls_l2_projection: the function has %d components, expected %d (%s, p)", prog.n_comps,
                   dim + 1, dim == 3 ? "u, v, w" : "u, v");
  if (prog.n_vars != dim + 1)
    return set_err(GLS_EINVAL, "gls_l2_projection: the function has %d variables, expected %d (%s, t)", prog.n_vars,
                   dim + 1, dim == 3 ? "x, y, z" : "x, y");
  if (!gls::mass_supported(dim, c->k, c->kp, c->map_degree, prog.max_stack))
    return set_err(GLS_EINVAL, "gls_l2_projection: no launch shape for an operand stack of %d entries", prog.max_stack);
  const int64_t n = c->n_dofs, nd = (int64_t)c->dir_dofs.n;
  hipStream_t s = c->stream;
  // the start vector: the Dirichlet values on the constrained DoFs, zero elsewhere
  HIP_TRY(gls::vec_fill(x, n, 0.0, s));
  if (nd) HIP_TRY(gls::vec_set_indexed(x, c->dir_dofs.p, c->dir_vals.p, nd, s));
  if (c->n_cells == 0 || n == 0) {
    HIP_TRY(hipStreamSynchronize(s));
    return GLS_OK;
  }
  const int64_t ns = (n + 1) / 2 * 2;  // the work vectors 16 bytes apart: one dot kernel whatever n
  if (p->vec.n != (size_t)(6 * ns)) GLS_TRY(p->vec.alloc((size_t)(6 * ns)));
  double *b = p->vec.p, *r = b + ns, *z = r + ns, *pd = z + ns, *Ap = pd + ns, *d = Ap + ns;
  GLS_TRY(mass_launch(c, p, gls::kMassRhs, nullptr, &prog, time));
  GLS_TRY(mass_gather(c, p, b));
  HIP_TRY(gls::vec_copy(d, p->diag.p, n, s));
  if (nd) {  // r = b - M x0 on the free rows; the preconditioner is the identity on the others
    GLS_TRY(mass_apply(c, p, x, r, false));
    HIP_TRY(gls::vec_axpby(r, 1.0, b, -1.0, n, s));
    HIP_TRY(gls::vec_set_indexed(r, c->dir_dofs.p, nullptr, nd, s));
    HIP_TRY(gls::vec_set_const_indexed64(d, c->dir_dofs.p, nd, 1.0, s));
  } else {
    HIP_TRY(gls::vec_copy(r, b, n, s));
  }
  double bb = 0.0, h[2] = {0.0, 0.0};
  GLS_TRY(dots(c, p, b, 0, 1, b, &bb));
  HIP_TRY(gls::vec_div(z, r, d, n, s));
  HIP_TRY(gls::vec_copy(pd, z, n, s));
  GLS_TRY(dots(c, p, r, ns, 2, r, h));  // r . r, z . r
  double rr = h[0], rz = h[1];
  const double stop = kProjectionTolerance * kProjectionTolerance * std::max(bb, 1e-300);
  int it = 0;
  for (; it < kProjectionMaxIterations && rr > stop; ++it) {
    GLS_TRY(mass_apply(c, p, pd, Ap, true));
    double pAp = 0.0;
    GLS_TRY(dots(c, p, pd, 0, 1, Ap, &pAp));
    if (!(pAp > 0.0))
      return set_err(GLS_ENOCONV, "gls_l2_projection: conjugate gradients broke down after %d iterations (p . M p = %g)",
                     it, pAp);
    const double alpha = rz / pAp;
    HIP_TRY(gls::vec_axpy(x, alpha, pd, n, s));
    HIP_TRY(gls::vec_axpy(r, -alpha, Ap, n, s));
    HIP_TRY(gls::vec_div(z, r, d, n, s));
    GLS_TRY(dots(c, p, r, ns, 2, r, h));
    const double beta = h[1] / rz;
    rr = h[0];
    rz = h[1];
    HIP_TRY(gls::vec_axpby(pd, 1.0, z, beta, n, s));  // p = z + beta p
  }
  HIP_TRY(hipStreamSynchronize(s));
  const double rel = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
  if (info) {
    info->iterations = it;
    info->relative_residual = rel;
  }
  if (!(rr <= stop))
    return set_err(GLS_ENOCONV, "gls_l2_projection: no convergence in %d iterations (relative residual %.3e, tolerance %.1e)",
                   it, rel, kProjectionTolerance);
  return GLS_OK;
}

}  // extern "C"
