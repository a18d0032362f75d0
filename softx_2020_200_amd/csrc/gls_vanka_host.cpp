// gls_vanka_host.cpp -- host side of the additive cell-Vanka smoother (kernels: gls_vanka.hip; maps: gls_vanka_maps.cpp):
// the maps' upload at attach, the rebuild of the patch inverses once per Jacobian state (the linearization cache's
// epoch), the sweep, and the gls_vanka_* building blocks of the C-ABI.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gls_ctx.hpp"
#include "gls_vanka_maps.hpp"

using namespace gls_impl;

namespace gls_impl {

const char *vanka_refusal(const gls_ctx *c) {
  if (c->dim != 3) return "cell-Vanka smoother: 3D only";
  if (c->k != 2 || (c->kp != 1 && c->kp != 2) || c->nq1d != 3) return "cell-Vanka smoother: Q2-Q1 / Q2-Q2 with QGauss(3) only";
  if (c->use_brick) return "cell-Vanka smoother: not on brick (pencil) contexts; per-cell contexts only";
  // (the sibling-group bricks of a forest keep their linearization in the pencil layout, not in the per-cell cache)
  if (c->oct.on) return "cell-Vanka smoother: not on a forest context whose sibling groups run the brick (pencil) kernel";
  if (c->hang.on) return "cell-Vanka smoother: not on a level with hanging-node or slip lines";
  if (c->dist.on) return "cell-Vanka smoother: one rank only";
  return nullptr;
}

int vanka_attach(gls_ctx *c) {
  auto &V = c->vanka;
  if (V.on) return GLS_OK;
  if (const char *why = vanka_refusal(c)) return set_err(GLS_EINVAL, "%s", why);
  const int nv = 27, np = gls::ipow(c->kp + 1, 3);
  std::vector<int32_t> cv((size_t)c->n_cells * nv), cp;
  HIP_TRY(hipMemcpy(cv.data(), c->cell_vnodes.p, cv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (c->cell_pnodes.p) {
    cp.resize((size_t)c->n_cells * np);
    HIP_TRY(hipMemcpy(cp.data(), c->cell_pnodes.p, cp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  gls::VankaMaps M;
  std::string err;
  if (gls::build_vanka_maps(3, c->k, c->kp, c->n_cells, c->n_vnodes, c->n_pnodes, cv.data(), cp.empty() ? nullptr : cp.data(), M,
                            err) != 0)
    return set_err(GLS_EINVAL, "cell-Vanka smoother: %s", err.c_str());
  if (M.n_dofs != c->n_dofs) return set_err(GLS_EINVAL, "cell-Vanka smoother: DoF count of the maps differs");
  std::vector<uint8_t> con((size_t)c->n_dofs, 0);
  if (c->con_dofs.n) {
    std::vector<int64_t> cd(c->con_dofs.n);
    HIP_TRY(hipMemcpy(cd.data(), c->con_dofs.p, cd.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t d : cd)
      if (d >= 0 && d < c->n_dofs) con[(size_t)d] = 1;
  }
  GLS_TRY(ensure_element_maps(c));
  V.nd = M.nd;
  GLS_TRY(V.cell_dofs.upload(M.cell_dofs.data(), M.cell_dofs.size()));
  GLS_TRY(V.nb_off.upload(M.nb_off.data(), M.nb_off.size()));
  GLS_TRY(V.nb_cell.upload(M.nb_cell.data(), M.nb_cell.size()));
  GLS_TRY(V.ov_off.upload(M.ov_off.data(), M.ov_off.size()));
  GLS_TRY(V.ov_i.upload(M.ov_i.data(), M.ov_i.size()));
  GLS_TRY(V.ov_j.upload(M.ov_j.data(), M.ov_j.size()));
  GLS_TRY(V.con.upload(con.data(), con.size()));
  GLS_TRY(V.Ainv.alloc((size_t)c->n_cells * V.nd * gls::vanka_row_floats(V.nd)));
  GLS_TRY(V.flag.alloc((size_t)c->n_cells));
  V.valid = false;
  V.on = true;
  return GLS_OK;
}

// the element matrices at the Jacobian's state into K (the diagonal pass writes the linearization cache they read)
static int vanka_element(gls_ctx *c, double *K) {
  if (!c->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  if (!c->cq_valid || !c->diag_valid) {
    c->diag_valid = false;
    GLS_TRY(ensure_diag(c));
  }
  if (!c->cq_valid || c->cq.n != cell_cache_size(c)) return set_err(GLS_EINVAL, "cell-Vanka smoother: no linearization cache");
  gls::OpParams P = make_params(c, true);
  P.cq = c->cq.p;
  P.cq_mode = 2;
  HIP_TRY(gls::launch_vanka_element(c->kp, P, c->tables, K, c->stream));
  return GLS_OK;
}

int ensure_vanka(gls_ctx *c) {
  auto &V = c->vanka;
  GLS_TRY(vanka_attach(c));
  if (!c->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  if (!c->cq_valid || !c->diag_valid) {
    c->diag_valid = false;
    GLS_TRY(ensure_diag(c));
  }
  if (V.valid && V.epoch == c->cq_epoch) return GLS_OK;
  const bool verbose = std::getenv("GLS_MG_VERBOSE") != nullptr;
  if (verbose) HIP_TRY(hipStreamSynchronize(c->stream));
  const auto t0 = std::chrono::steady_clock::now();
  V.valid = false;
  // K and A live for the rebuild only (2 nd^2 doubles per cell, 4x the inverses): the sweeps read Ainv alone. A stays
  // when gls_vanka_patch_inverses asked for it (keep_A)
  const size_t nn = (size_t)c->n_cells * V.nd * V.nd;
  DevBuf<double> K, A;
  GLS_TRY(K.alloc(nn));
  GLS_TRY(A.alloc(nn));
  V.A.release();
  GLS_TRY(vanka_element(c, K.p));
  HIP_TRY(gls::launch_vanka_patch(c->n_cells, V.nd, K.p, V.nb_off.p, V.nb_cell.p, V.ov_off.p, V.ov_i.p, V.ov_j.p,
                                  V.cell_dofs.p, V.con.p, c->diag.p, A.p, c->stream));
  HIP_TRY(hipMemsetAsync(V.flag.p, 0, sizeof(int32_t) * (size_t)c->n_cells, c->stream));
  HIP_TRY(gls::launch_vanka_invert(c->n_cells, V.nd, A.p, V.Ainv.p, V.flag.p, c->stream));
  std::vector<int32_t> flag((size_t)c->n_cells);
  HIP_TRY(hipMemcpyAsync(flag.data(), V.flag.p, sizeof(int32_t) * flag.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (also: K and A are free to go)
  if (V.keep_A) V.A = std::move(A);
  int64_t nbad = 0, first = -1;
  for (size_t i = 0; i < flag.size(); ++i)
    if (flag[i]) {
      if (first < 0) first = (int64_t)i;
      ++nbad;
    }
  if (nbad)
    return set_err(GLS_EINVAL, "cell-Vanka smoother: the patch matrix of cell %lld is singular or not finite (%lld such cells)",
                   (long long)first, (long long)nbad);
  V.setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (verbose)
    std::printf("mg: cell-Vanka setup %d cells x %d DoFs: %.3f ms (element matrices, patch assembly, inversion)\n", c->n_cells,
                V.nd, 1e3 * V.setup_s);
  V.epoch = c->cq_epoch;
  V.valid = true;
  return GLS_OK;
}

int vanka_sweep(gls_ctx *c, double *x, const double *b, double *y, double omega, bool x_zero) {
  auto &V = c->vanka;
  GLS_TRY(ensure_vanka(c));
  const double *r = b;
  if (x_zero) {
    HIP_TRY(gls::vec_fill(x, c->n_dofs, 0.0, c->stream));
  } else {
    GLS_TRY(gls_jacobian_apply(c, x, y));
    HIP_TRY(gls::vec_axpby(y, 1.0, b, -1.0, c->n_dofs, c->stream));  // y = b - A x
    r = y;
  }
  HIP_TRY(gls::launch_vanka_apply(c->n_cells, V.nd, V.Ainv.p, V.cell_dofs.p, r, c->ev.p, c->stream));
  HIP_TRY(gls::launch_vanka_update(x, c->ev.p, c->ev_voff.p, c->ev_vslot.p, c->n_vnodes, c->ev_poff.p, c->ev_pslot.p,
                                   c->n_pnodes, c->dim, omega, c->stream));
  return GLS_OK;
}

}  // namespace gls_impl

extern "C" {

int gls_vanka_sizes(gls_ctx *c, int *nd, int *row_floats) {
  GLS_TRY(check_ctx(c));
  if (const char *why = vanka_refusal(c)) return set_err(GLS_EINVAL, "%s", why);
  const int n = 81 + gls::ipow(c->kp + 1, 3);
  if (nd) *nd = n;
  if (row_floats) *row_floats = gls::vanka_row_floats(n);
  return GLS_OK;
}

int gls_vanka_element_matrices(gls_ctx *c, double *K) {
  GLS_TRY(check_ctx(c));
  if (!K) return set_err(GLS_EINVAL, "gls_vanka_element_matrices: K is null");
  if (const char *why = vanka_refusal(c)) return set_err(GLS_EINVAL, "%s", why);
  return vanka_element(c, K);
}

int gls_vanka_patch_inverses(gls_ctx *c, double *A, float *Ainv) {
  GLS_TRY(check_ctx(c));
  GLS_TRY(vanka_attach(c));
  if (A && !c->vanka.keep_A) {  // from now on the rebuilds keep the patch matrices
    c->vanka.keep_A = true;
    c->vanka.valid = false;
  }
  GLS_TRY(ensure_vanka(c));
  const auto &V = c->vanka;
  const size_t nn = (size_t)c->n_cells * V.nd * V.nd;
  if (A) HIP_TRY(hipMemcpyAsync(A, V.A.p, sizeof(double) * nn, hipMemcpyDeviceToDevice, c->stream));
  if (Ainv)
    HIP_TRY(hipMemcpyAsync(Ainv, V.Ainv.p, sizeof(float) * (size_t)c->n_cells * V.nd * gls::vanka_row_floats(V.nd),
                           hipMemcpyDeviceToDevice, c->stream));
  return GLS_OK;
}

int gls_vanka_sweep(gls_ctx *c, double *x, const double *b, double omega) {
  GLS_TRY(check_ctx(c));
  if (!x || !b || x == b) return set_err(GLS_EINVAL, "gls_vanka_sweep: x / b null or aliased");
  if (!(omega > 0.0)) omega = 0.8;
  if (const char *why = vanka_refusal(c)) return set_err(GLS_EINVAL, "%s", why);
  if (c->vanka.r.n != (size_t)c->n_dofs) GLS_TRY(c->vanka.r.alloc((size_t)c->n_dofs));
  return vanka_sweep(c, x, b, c->vanka.r.p, omega);
}

int gls_vanka_detach(gls_ctx *c) {
  GLS_TRY(check_ctx(c));
  if (c->vanka.smooth) return set_err(GLS_EINVAL, "gls_vanka_detach: the attached multigrid smooths with it (gls_mg_detach)");
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->vanka = gls_ctx::Vanka();
  return GLS_OK;
}

}  // extern "C"
