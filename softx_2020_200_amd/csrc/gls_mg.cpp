// gls_mg.cpp -- the geometric multigrid V-cycle (right preconditioner): the levels' re-discretisation and the probing
// of the coarsest matrix (mg_prepare), the transfers, the two V-cycles, the HIP-graph coarse sweeps, and the attach /
// detach entry points of include/gls_native.h. The coarsest level's direct solve is gls_mg_coarse.cpp's; the
// operator side the cycle calls (J.v, smoother sweeps, ghost exchange) is gls_api.cpp's.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gls_ctx.hpp"

using namespace gls_impl;

// --------------------------------------------------------------------------------------------
// Geometric multigrid V-cycle (right preconditioner). Levels are nested hyper_cube meshes; the
// coarse operators are the same GLS Jacobian re-discretised on the coarse mesh at the injected
// state (Galerkin-free, matrix-free), smoothed by damped Jacobi on their own diagonals.
// --------------------------------------------------------------------------------------------
namespace {
enum { MB_U = 0, MB_U1, MB_U2, MB_U3, MB_B, MB_X, MB_Y, MB_BOX, MB_N };
double *mgbuf(gls_ctx *c, int l, int which) { return c->mg.bufs[(size_t)l * MB_N + which]->p; }
int64_t mg_nbox(const gls_ctx *c, int l) {
  const auto &d = c->mg.dims[(size_t)l];
  return (int64_t)d[0] * d[1] * d[2];
}
// level-l local vector -> box lattice layout (identity on a single GPU: returns loc itself)
const double *mg_to_box(gls_ctx *c, int l, const double *loc, bool owned_only) {
  if (!c->mg.boxed) return loc;
  gls_ctx *g = c->mg.lev[(size_t)l];
  double *box = mgbuf(c, l, MB_BOX);
  if (gls::mg_box_gather(loc, box, g->lat.map.p, mg_nbox(c, l), g->n_vnodes, owned_only ? g->dist.n_owned : -1,
                         c->stream) != hipSuccess)
    return nullptr;
  return box;
}
// where a transfer writing level-l data must put it (the box buffer, or loc itself)
double *mg_box_target(gls_ctx *c, int l, double *loc) { return c->mg.boxed ? mgbuf(c, l, MB_BOX) : loc; }
int mg_from_box(gls_ctx *c, int l, double *loc) {
  if (!c->mg.boxed) return GLS_OK;
  gls_ctx *g = c->mg.lev[(size_t)l];
  HIP_TRY(gls::mg_box_scatter(mgbuf(c, l, MB_BOX), loc, g->lat.map.p, mg_nbox(c, l), g->n_vnodes, c->stream));
  return GLS_OK;
}

// injected coarse state (every second lattice node); history likewise
int mg_inject_level(gls_ctx *c, int l, const double *fine, double *coarse) {
  if (c->mg.csr) {  // general hierarchy: the fine value at each coarse DoF's position (hanging values follow)
    const auto &X = *c->mg.xfer[(size_t)l - 1];
    HIP_TRY(gls::vec_pack_dofs(fine, X.inj.p, X.nc, coarse, c->stream));
    gls_ctx *g = c->mg.lev[(size_t)l];
    if (g->hang.on)
      HIP_TRY(gls::vec_csr_gather_set(coarse, coarse, g->hang.dof.p, g->hang.off.p, g->hang.master.p, g->hang.w.p,
                                      (int64_t)g->hang.dof.n, c->stream));
    return GLS_OK;
  }
  const double *fb = mg_to_box(c, l - 1, fine, false);
  if (!fb) return set_err(GLS_EHIP, "mg box gather failed");
  HIP_TRY(gls::mg_inject(fb, mg_box_target(c, l, coarse), c->mg.dims[(size_t)l - 1].data(), c->mg.dims[(size_t)l].data(),
                         c->stream));
  return mg_from_box(c, l, coarse);
}

// the replica's copy of a fine-level state vector: each replica DoF takes its injection source's value on
// the one rank that owns that fine DoF (0 elsewhere), then the sum over ranks
int rep2_inject(gls_ctx *c, const double *loc, double *glob) {
  auto &mg = c->mg;
  const int64_t ng = mg.rep2->n_dofs, ni = (int64_t)mg.r2inj_c.n;
  HIP_TRY(gls::vec_fill(glob, ng, 0.0, c->stream));
  if (ni) {
    HIP_TRY(gls::vec_pack_dofs(loc, mg.r2inj_f.p, ni, mg.rep_tmp.p, c->stream));
    HIP_TRY(gls::vec_unpack_dofs(glob, mg.r2inj_c.p, ni, mg.rep_tmp.p, c->stream));
  }
  return dist_allreduce_vector(c, glob, ng);
}
// glob (replica numbering, every rank) = the coarsest distributed level's vector loc: each rank scatters
// its owned rows into a zeroed copy, then the sum over ranks through that level's transport
int replica_gather(gls_ctx *c, const double *loc, double *glob) {
  auto &mg = c->mg;
  const int64_t ng = mg.replica->n_dofs, no = (int64_t)mg.rep_own_loc.n;
  hipStream_t s = c->stream;
  HIP_TRY(gls::vec_fill(glob, ng, 0.0, s));
  if (no) {
    HIP_TRY(gls::vec_pack_dofs(loc, mg.rep_own_loc.p, no, mg.rep_tmp.p, s));
    HIP_TRY(gls::vec_unpack_dofs(glob, mg.rep_own_glob.p, no, mg.rep_tmp.p, s));
  }
  const int rc = dist_allreduce_vector(mg.lev.back(), glob, ng);
  return rc == GLS_ECOMM ? set_err(GLS_ECOMM, "replica all-reduce failed") : rc;
}

// the direct coarse solve's matrix by colored probing on a per-cell level (mg.probe_ilu; brick levels and
// distributed or nested contexts: one J.v per column): the ILU structure (CM order, fill 0, one block) is attached once
int mg_probe_setup(gls_ctx *c, gls_ctx *g) {
  auto &mg = c->mg;
  mg.probe_ilu = nullptr;
  if ((g->use_brick && g->use_qdata) || g->dist.on || g->mg.on || g->ilu.on)
    return GLS_OK;
  GLS_TRY(gls_ilu_set_options(g, GLS_ILU_ORDER_CM, 0));
  GLS_TRY(gls_ilu_attach(g, 0, 0.0, 1.0));
  g->ilu.probe_only = true;
  mg.ilu_levels.push_back(g);  // detached with the multigrid
  GLS_TRY(mg.coarse.pinv.alloc((size_t)g->n_dofs));
  mg.probe_ilu = g;
  return GLS_OK;
}
// ---- the band route of the direct coarse solve (coarse_direct 2, or 1 above kDirectMax): the FP32 matrix in
// block-tridiagonal storage, filled from the probing ILU's CSR (gls_band_lu.hpp)
bool band_route_wanted(const gls_mg_params *p, const gls_ctx *g) {
  return p->coarse_direct == 2 || (p->coarse_direct == 1 && g->n_dofs > kDirectMax);
}
// the panels plus the CSR may take this fraction of the free device memory at attach
constexpr double kBandMemFraction = 0.5;
int band_fits(const char *who, int64_t n, size_t panel_bytes, size_t csr_bytes, const char *bound) {
  size_t fr = 0, tot = 0;
  HIP_TRY(hipMemGetInfo(&fr, &tot));
  double limit = kBandMemFraction * (double)fr;
  if (const char *e = std::getenv("GLS_MG_BAND_MAX_BYTES")) limit = std::min(limit, std::atof(e));  // a caller's lower cap
  if ((double)panel_bytes + (double)csr_bytes <= limit) return GLS_OK;
  return set_err(GLS_EINVAL, "%s: band storage of the coarsest level (n %lld) needs %s%zu bytes of panels + %zu of CSR, "
                             "above the limit of %.0f (half of the %zu bytes free, or GLS_MG_BAND_MAX_BYTES)", who,
                 (long long)n, bound, panel_bytes, csr_bytes, limit, fr);
}
// what can be refused before anything is detached: a coarsest level g that mg_probe_setup would not probe through an
// ILU CSR (an ILU attached by this context's own multigrid goes with the detach), and panels that cannot fit even
// at the narrowest block (the bandwidths are known only once the probing ILU is attached: mg_coarse_setup)
int band_precheck(const char *who, gls_ctx *c, const gls_mg_params *p, gls_ctx *g) {
  if (!g || !band_route_wanted(p, g)) return GLS_OK;
  const auto &own = c->mg.ilu_levels;
  const char *why = g->use_brick && g->use_qdata ? "it runs the brick kernels and is probed by them"
                    : g->dist.on                 ? "it is distributed"
                    : g->mg.on                   ? "it has a hierarchy of its own"
                    : g->ilu.on && std::find(own.begin(), own.end(), g) == own.end()
                        ? "it has an ILU of its own and is probed column by column"
                        : nullptr;
  if (why)
    return set_err(GLS_EINVAL, "%s: coarse_direct %d on %lld DoFs takes band storage, which needs a coarsest level probed "
                               "through its ILU CSR: %s", who, p->coarse_direct, (long long)g->n_dofs, why);
  return band_fits(who, g->n_dofs, sizeof(float) * (size_t)(3 * g->n_dofs * kBandSub), 0, "at least ");
}
int mg_probe_band(gls_ctx *c, gls_ctx *g);
// the direct coarse solve's storage and probing pattern on the coarsest level g
int mg_coarse_setup(const char *who, gls_ctx *c, gls_ctx *g, bool band) {
  auto &mg = c->mg;
  if (!band) {
    GLS_TRY(mg.coarse.init(g->n_dofs));
    return mg_probe_setup(c, g);
  }
  GLS_TRY(mg_probe_setup(c, g));
  if (mg.probe_ilu != g) return set_err(GLS_EINVAL, "%s: band storage needs a coarsest level probed through its ILU CSR", who);
  GLS_TRY(mg_probe_band(c, g));  // the bandwidths of the CSR's Cuthill-McKee order
  const char *e = std::getenv("GLS_MG_BAND_BLOCK");  // the block width (a multiple of 128; default: by the band)
  const int64_t block = e ? std::atoll(e) : 0;
  BandLayout L;
  if (const char *why = band_layout(g->n_dofs, mg.coarse.band.bl, mg.coarse.band.bu, block, &L))
    return set_err(GLS_EINVAL, "%s: coarse band storage: %s", who, why);
  const size_t csr = (size_t)g->ilu.nnz * (sizeof(double) + sizeof(int32_t)) + ((size_t)g->n_dofs + 1) * sizeof(int64_t);
  GLS_TRY(band_fits(who, g->n_dofs, sizeof(float) * (size_t)L.n_floats, csr, ""));
  return mg.coarse.init_band(g->n_dofs, block);
}
// first step of the preparation: the levels re-discretised at the Jacobian's state (the frozen snapshot under
// skip_newton): injected state and history, time data, diagonal; the replicas take theirs summed over ranks
int mg_prepare_levels(gls_ctx *c) {
  auto &mg = c->mg;
  const int L = (int)mg.lev.size();
  const bool fz = c->jf.on;
  const double *ju = fz ? c->jf.u.p : c->u;
  const double *jh[3] = {fz ? (c->jf.has[0] ? c->jf.h[0].p : nullptr) : c->u1,
                         fz ? (c->jf.has[1] ? c->jf.h[1].p : nullptr) : c->u2,
                         fz ? (c->jf.has[2] ? c->jf.h[2].p : nullptr) : c->u3};
  const int jscheme = fz ? c->jf.scheme : c->scheme;
  const double *jts = fz ? c->jf.ts : c->time_steps;
  for (int l = 1; l < L; ++l) {
    gls_ctx *g = mg.lev[l];
    const double *fu = l == 1 ? ju : mgbuf(c, l - 1, MB_U);
    const double *fh[3] = {l == 1 ? jh[0] : (jh[0] ? mgbuf(c, l - 1, MB_U1) : nullptr),
                           l == 1 ? jh[1] : (jh[1] ? mgbuf(c, l - 1, MB_U2) : nullptr),
                           l == 1 ? jh[2] : (jh[2] ? mgbuf(c, l - 1, MB_U3) : nullptr)};
    GLS_TRY(mg_inject_level(c, l, fu, mgbuf(c, l, MB_U)));
    GLS_TRY(gls_apply_dirichlet(g, mgbuf(c, l, MB_U)));
    double *gh[3] = {nullptr, nullptr, nullptr};
    for (int h = 0; h < 3; ++h)
      if (fh[h]) {
        gh[h] = mgbuf(c, l, MB_U1 + h);
        GLS_TRY(mg_inject_level(c, l, fh[h], gh[h]));
      }
    g->viscosity = c->viscosity;
    GLS_TRY(gls_set_time(g, jscheme, jts));
    GLS_TRY(gls_set_state(g, mgbuf(c, l, MB_U), gh[0], gh[1], gh[2]));
    GLS_TRY(ensure_diag(g));
  }
  if (mg.rep_csr) {  // the replica hierarchy takes the fine state (injected, summed over ranks) and time data
    gls_ctx *r = mg.rep2;
    const double *st[4] = {ju, jh[0], jh[1], jh[2]};
    for (int i = 0; i < 4; ++i)
      if (st[i]) GLS_TRY(rep2_inject(c, st[i], mg.rep_u[i].p));
    GLS_TRY(gls_apply_dirichlet(r, mg.rep_u[0].p));
    r->viscosity = c->viscosity;
    GLS_TRY(gls_set_time(r, jscheme, jts));
    GLS_TRY(gls_set_state(r, mg.rep_u[0].p, st[1] ? mg.rep_u[1].p : nullptr, st[2] ? mg.rep_u[2].p : nullptr,
                          st[3] ? mg.rep_u[3].p : nullptr));
  }
  if (mg.replica) {  // the replica takes the coarsest distributed level's state (gathered) and time data
    gls_ctx *g = mg.lev[(size_t)L - 1], *r = mg.replica;
    const double *st[4] = {g->u, g->u1, g->u2, g->u3};
    for (int i = 0; i < 4; ++i)
      if (st[i]) GLS_TRY(replica_gather(c, st[i], mg.rep_u[i].p));
    r->viscosity = c->viscosity;
    GLS_TRY(gls_set_time(r, jscheme, jts));
    GLS_TRY(gls_set_state(r, mg.rep_u[0].p, st[1] ? mg.rep_u[1].p : nullptr, st[2] ? mg.rep_u[2].p : nullptr,
                          st[3] ? mg.rep_u[3].p : nullptr));
  }
  return GLS_OK;
}

// second step, the coarse matrix A = J_coarse probed into the dense array by one of three routes. Brick levels: all
// unit vectors of a batch in one launch
int mg_probe_brick(gls_ctx *c, gls_ctx *g, double *A) {
  const int64_t n = g->n_dofs;
  GLS_TRY(ensure_diag(g));
  GLS_TRY(ensure_qdata(g));
  gls::OpParams P = make_params(g, true);
  P.qd = g->qdata.p;
  HIP_TRY(hipMemsetAsync(A, 0, sizeof(double) * (size_t)(n * n), c->stream));
  const int batch = 4096;
  for (int64_t j0 = 0; j0 < n; j0 += batch) {
    const int nb = (int)std::min<int64_t>(batch, n - j0);
    P.y = A + j0 * n;
    HIP_TRY(gls::launch_brick_probe(g->k, P, g->tables, j0, nb, c->stream));
    HIP_TRY(gls::mg_probe_fix(A + j0 * n, n, j0, nb, g->con_dofs.p, (int64_t)g->con_dofs.n, g->diag.p, c->stream));
  }
  return GLS_OK;
}
// the FP32 range keeps the probing ILU's Cuthill-McKee order (banded): the bandwidths from its pattern, the identity
// permutation and the first pressure DoF's row, once
int mg_probe_band(gls_ctx *c, gls_ctx *g) {
  auto &cs = c->mg.coarse;
  const auto &I = g->ilu;
  const int64_t n = g->n_dofs;
  std::vector<int64_t> rp((size_t)n + 1);
  std::vector<int32_t> cl((size_t)I.nnz), pm((size_t)n), id((size_t)n);
  HIP_TRY(hipMemcpy(rp.data(), I.rowp.p, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cl.data(), I.col.p, sizeof(int32_t) * cl.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pm.data(), I.perm.p, sizeof(int32_t) * pm.size(), hipMemcpyDeviceToHost));
  int64_t bl = 0, bu = 0;
  for (int64_t r = 0; r < n; ++r)
    for (int64_t e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) {
      bl = std::max<int64_t>(bl, r - cl[(size_t)e]);
      bu = std::max<int64_t>(bu, cl[(size_t)e] - r);
    }
  for (int64_t i = 0; i < n; ++i) id[(size_t)i] = (int32_t)i;
  GLS_TRY(cs.ident.upload(id.data(), id.size()));
  cs.band = {bl, bu, pm[(size_t)((int64_t)g->dim * g->n_vnodes)]};
  if (std::getenv("GLS_MG_VERBOSE"))
    std::printf("mg: coarse matrix n=%lld in Cuthill-McKee order: bandwidths %lld / %lld\n", (long long)n, (long long)bl,
                (long long)bu);
  return GLS_OK;
}
// per-cell levels: colored batched probes into the probing ILU's CSR (mg_probe_setup), then dense; *banded: in the
// CSR's own order
int mg_probe_ilu_csr(gls_ctx *c, gls_ctx *g, double *A, bool *banded) {
  auto &cs = c->mg.coarse;
  const int64_t n = g->n_dofs;
  GLS_TRY(ensure_diag(g));
  GLS_TRY(ilu_probe(g));
  HIP_TRY(hipMemsetAsync(A, 0, sizeof(double) * (size_t)(n * n), c->stream));
  const auto &I = g->ilu;
  *banded = n > kDirectSmall;
  if (*banded && cs.band.bl < 0) GLS_TRY(mg_probe_band(c, g));
  HIP_TRY(gls::csr_to_dense(A, I.rowp.p, I.col.p, I.val.p, *banded ? cs.ident.p : I.perm.p, cs.pinv.p, n, c->stream));
  return GLS_OK;
}
// any other level: one J.v per column
int mg_probe_columns(gls_ctx *c, gls_ctx *g, double *A) {
  const int64_t n = g->n_dofs;
  double *unit = c->mg.coarse.unit.p;
  HIP_TRY(gls::vec_fill(unit, n, 0.0, c->stream));
  for (int64_t j = 0; j < n; ++j) {
    HIP_TRY(gls::mg_unit_step(unit, j, c->stream));
    GLS_TRY(gls_jacobian_apply(g, unit, A + j * n));
  }
  return GLS_OK;
}
}  // namespace

namespace gls_impl {  // declared in gls_ctx.hpp
int mg_prepare(gls_ctx *c) {
  auto &mg = c->mg;
  if (!mg.dirty) return GLS_OK;
  // (its buffers are re-probed below; a failed check of the band route's superseded factor is not this state's error)
  if (const int rc = mg.coarse.finish(c->stream); rc < 0 && !(mg.coarse.band_store && rc == GLS_EINVAL)) return rc;
  if (std::getenv("GLS_MG_VERBOSE")) (void)hipStreamSynchronize(c->stream);  // host wall time of the phases
  const auto t0 = CoarseSolve::Clock::now();
  GLS_TRY(mg_prepare_levels(c));
  mg.coarse.ok = false;
  if (mg.direct && mg.coarse.band_store) {  // band storage: the probed CSR itself is the matrix, no dense array
    gls_ctx *g = mg.rep_csr ? mg.rep2 : mg.lev.back();
    GLS_TRY(ensure_diag(g));
    GLS_TRY(ilu_probe(g));
    const auto &I = g->ilu;
    GLS_TRY(mg.coarse.factor_band(c->stream, I.rowp.p, I.col.p, I.val.p, (int64_t)g->dim * g->n_vnodes, t0));
  } else if (mg.direct) {
    // coarsest level: the last one, or the whole-mesh replica below a distributed fine level (rep_csr)
    gls_ctx *g = mg.rep_csr ? mg.rep2 : mg.lev.back();
    double *A = mg.coarse.matrix();
    bool banded = false;
    if (g->use_brick && g->use_qdata) GLS_TRY(mg_probe_brick(c, g, A));
    else if (mg.probe_ilu == g && g->ilu.on) GLS_TRY(mg_probe_ilu_csr(c, g, A, &banded));
    else GLS_TRY(mg_probe_columns(c, g, A));
    // third step: factored with the first pressure DoF pinned
    GLS_TRY(mg.coarse.factor(c->stream, (int64_t)g->dim * g->n_vnodes, banded, t0));
  }
  // the cell-Vanka levels' patch inverses at this state (where the ILU smoothers refactor): a singular patch is
  // reported here and leaves the hierarchy dirty
  for (auto *g : mg.lev)
    if (g->vanka.smooth) GLS_TRY(ensure_vanka(g));
  mg.dirty = false;
  return GLS_OK;
}
}  // namespace gls_impl

namespace {
// coarse rhs bc (level l+1) = R y (y on level l): restrict the owned rows, export-add coarse ghost rows
int mg_restrict(gls_ctx *c, int l, const double *y, double *bc) {
  auto &mg = c->mg;
  gls_ctx *h = mg.lev[(size_t)l + 1];
  hipStream_t s = c->stream;
  if (mg.csr) {
    const auto &X = *mg.xfer[(size_t)l];
    HIP_TRY(gls::vec_csr_spmv(bc, y, X.roff.p, X.rcol.p, X.rw.p, X.nc, false, s, X.rlane));
    (void)h;
    return GLS_OK;
  }
  const double *yb = mg_to_box(c, l, y, true);
  if (!yb) return set_err(GLS_EHIP, "mg box gather failed");
  {
    const auto &T = *mg.taps[(size_t)l];
    const int32_t *ti[3] = {T.ri[0].p, T.ri[1].p, T.ri[2].p}, *tc[3] = {T.rc[0].p, T.rc[1].p, T.rc[2].p};
    const double *tw[3] = {T.rw[0].p, T.rw[1].p, T.rw[2].p};
    if (T.two_pass)
      HIP_TRY(gls::mg_transfer_2pass(yb, mg_box_target(c, l + 1, bc), mg.dims[l].data(), mg.dims[l + 1].data(), 1, ti,
                                     tw, tc, mg.xwork.p, s, 0, T.wrap ? 1 : 0));
    else
      HIP_TRY(gls::mg_transfer3d(yb, mg_box_target(c, l + 1, bc), mg.dims[l].data(), mg.dims[l + 1].data(), ti, tw,
                                 tc, s));
  }
  GLS_TRY(mg_from_box(c, l + 1, bc));
  GLS_TRY(dist_export_add(h, bc));
  return GLS_OK;
}

// y (level l) = P xc (xc on level l+1; its ghost values are imported first); add: y += P xc
// (single rank, two-pass transfer only: the caller checks mg_prolong_add_ok)
bool mg_prolong_add_ok(gls_ctx *c, int l) {
  if (c->mg.csr) return false;  // general hierarchies: P xc, constrained rows zeroed, then added
  return !c->mg.boxed && c->mg.taps[(size_t)l]->two_pass && std::getenv("GLS_MG_NO_FUSE") == nullptr;
}
int mg_prolong(gls_ctx *c, int l, double *xc, double *y, bool add = false) {
  auto &mg = c->mg;
  gls_ctx *h = mg.lev[(size_t)l + 1];
  hipStream_t s = c->stream;
  if (mg.csr) {
    const auto &X = *mg.xfer[(size_t)l];
    HIP_TRY(gls::vec_csr_spmv(y, xc, X.poff.p, X.pcol.p, X.pw.p, X.nf, add, s, X.plane));
    return GLS_OK;
  }
  GLS_TRY(dist_import(h, xc));
  const double *xb = mg_to_box(c, l + 1, xc, false);
  if (!xb) return set_err(GLS_EHIP, "mg box gather failed");
  {
    const auto &T = *mg.taps[(size_t)l];
    const int32_t *ti[3] = {T.pi[0].p, T.pi[1].p, T.pi[2].p}, *tc[3] = {T.pc[0].p, T.pc[1].p, T.pc[2].p};
    const double *tw[3] = {T.pw[0].p, T.pw[1].p, T.pw[2].p};
    if (T.two_pass)
      HIP_TRY(gls::mg_transfer_2pass(xb, mg_box_target(c, l, y), mg.dims[l + 1].data(), mg.dims[l].data(), 0, ti, tw,
                                     tc, mg.xwork.p, s, add ? 1 : 0, T.wrap ? 1 : 0));
    else if (add)
      return set_err(GLS_EINVAL, "mg_prolong: accumulate needs the two-pass transfer");
    else
      HIP_TRY(gls::mg_transfer3d(xb, mg_box_target(c, l, y), mg.dims[l + 1].data(), mg.dims[l].data(), ti, tw, tc, s));
  }
  GLS_TRY(mg_from_box(c, l, y));
  return GLS_OK;
}

// The residual and its restriction in one J.v launch (single rank, FP32 smoothing on the cube's Q2 bricks,
// nested lattice levels with the two-pass taps): the pencil J.v restricts each brick's part of b - A x to the
// brick's coarse cell, and one sum over the coarse lattice forms the coarse right-hand side with its constrained
// rows zeroed. The fine residual vector, the slab, its sum and both restriction passes are not needed.
// GLS_MG_FUSE_TRANSFER=0 (read per call) or GLS_MG_NO_FUSE keep the separate launches.
bool mg_fused_restrict_ok(gls_ctx *c, int l) {
  auto &mg = c->mg;
  if (l < 0 || l + 1 >= (int)mg.lev.size() || mg.csr || mg.boxed || (size_t)l >= mg.taps.size()) return false;
  const char *e = std::getenv("GLS_MG_FUSE_TRANSFER");
  if ((e && std::atoi(e) == 0) || std::getenv("GLS_MG_NO_FUSE") != nullptr) return false;
  gls_ctx *g = mg.lev[(size_t)l], *h = mg.lev[(size_t)l + 1];
  const auto &T = *mg.taps[(size_t)l];
  const int64_t nc1 = 2 * (int64_t)g->cube_nb1 + 1;
  return T.two_pass && T.q2_brick && g->smooth_f32 && g->use_brick && g->use_qdata && !g->use_colors && !g->dist.on &&
         !g->hang.on && !g->oct.on && g->k == 2 && g->cube_nb1 > 0 && g->cube_nb1 < 1024 && g->use_slab && !g->srf &&
         gls::pencil_enabled() && gls::brick_fused_jacobi_supported(g->k) && !h->dist.on && !h->hang.on &&
         h->n_vnodes == nc1 * nc1 * nc1 && g->stream == c->stream;
}
// bc (level l + 1) = R (b - A x) with the constrained coarse rows zeroed (x, b on level l). first_omega > 0
// (first_sweep_fusable levels): x is not read but formed and stored as the first damped-Jacobi sweep from 0,
// as in jacobian_apply_f32. xc0 (level l + 1, with that level's damping): the sum also stores that level's first
// damped-Jacobi sweep from 0, xc0 = 0 + omega_c bc / D_c
int mg_residual_restrict_fused(gls_ctx *c, int l, double *x, const double *b, double *bc, double first_omega = 0.0,
                               double *xc0 = nullptr, double omega_c = 0.0) {
  gls_ctx *g = c->mg.lev[(size_t)l], *h = c->mg.lev[(size_t)l + 1];
  if (!g->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  GLS_TRY(ensure_diag(g));
  GLS_TRY(ensure_qdata32(g, !g->smooth_oseen));
  if (xc0) GLS_TRY(ensure_diag(h));
  gls::OpParams P = make_params(g, true);
  P.qdf = g->qdata32.p;
  P.oseen = g->smooth_oseen ? 1 : 0;
  P.v = x;
  P.rb = b;
  P.cube_nb1 = g->cube_nb1;
  if (first_omega > 0.0) {
    P.jx0 = x;
    P.jd = g->diag.p;
    P.jomega = first_omega;
  }
  P.slab = brick_slab(g);  // holds the bricks' coarse element vectors [brick][27][4] here (the slab is larger)
  if (!P.slab) return set_err(GLS_EHIP, "brick slab allocation failed");
  {
    TimedLaunch t(g, 4);
    HIP_TRY(gls::launch_pencil_jv_restrict(P, g->tables, c->stream));
  }
  TimedLaunch t(g, 5);
  HIP_TRY(gls::brick_restrict_sum_cube(g->cube_nb1, P.slab, h->n_vnodes, bc, h->vmask.p, c->stream, xc0,
                                       xc0 ? h->diag.p : nullptr, omega_c));
  return GLS_OK;
}

// The prolongation inside the first post-sweep (same level pairs as the fused restriction, and the coarse level a
// verified hyper_cube lattice too): the fused damped-Jacobi sweep's J.v gathers x + P xc, interpolating each
// brick's coarse cell in LDS, and hands that value at the brick-surface nodes to the slab sum through the level's
// scratch vector, so the two transfer launches and their passes over x are not needed. The hard-coded Q2 weights are those checked against the level
// pair's tap tables at attach (Taps::q2_brick). GLS_MG_FUSE_PROLONG=0 (read per call) or GLS_MG_NO_FUSE keep the
// separate launches.
bool mg_fused_prolong_ok(gls_ctx *c, int l) {
  auto &mg = c->mg;
  if (l < 0 || l + 1 >= (int)mg.lev.size() || mg.csr || mg.boxed || (size_t)l >= mg.taps.size() || !mg_prolong_add_ok(c, l))
    return false;
  const char *e = std::getenv("GLS_MG_FUSE_PROLONG");
  if (e && std::atoi(e) == 0) return false;
  gls_ctx *g = mg.lev[(size_t)l], *h = mg.lev[(size_t)l + 1];
  const auto &T = *mg.taps[(size_t)l];
  const int64_t nc1 = 2 * (int64_t)g->cube_nb1 + 1;
  const bool ilu_smooth = mg.ilu_smooth && g->ilu.on && !g->ilu.probe_only;
  return T.two_pass && T.q2_brick && mg.lpost[(size_t)l] >= 1 && !ilu_smooth && g->smooth_f32 && g->use_brick &&
         g->use_qdata && !g->use_colors && !g->dist.on && !g->hang.on && !g->oct.on && g->k == 2 && g->cube_nb1 > 0 &&
         g->cube_nb1 < 1024 && g->use_slab && brick_slab(g) && !g->srf && gls::pencil_enabled() &&
         gls::brick_fused_jacobi_supported(g->k) && !h->dist.on && !h->hang.on && h->cube_nb1 > 0 &&
         g->cube_nb1 == 2 * h->cube_nb1 && h->n_vnodes == nc1 * nc1 * nc1 && g->stream == c->stream;
}

// coarsest level by HIP graph (opt-in, GLS_MG_GRAPH=1: measured at 128^3, 138.0 vs 138.6 ms per
// Newton step -- the coarse sweeps are bound by the kernels' own latency, not by launch overhead,
// profiles/r01_coarse_graph_bench.txt): one rank, fused brick sweeps, the level's own b / x buffers (the
// captured launches bake in their pointers and this state's OpParams; mg_prepare drops the graph)
bool coarse_graph_eligible(gls_ctx *c, gls_ctx *g, const double *b, const double *x) {
  const int l = (int)c->mg.lev.size() - 1;
  return !c->mg.cgraph_failed && !c->mg.boxed && !g->dist.on && !g->hang.on && g->use_brick && g->use_qdata &&
         brick_slab(g) && gls::brick_fused_jacobi_supported(g->k) && g->stream == c->stream &&
         b == mgbuf(c, l, MB_B) && x == mgbuf(c, l, MB_X) && std::getenv("GLS_MG_NO_FUSE") == nullptr &&
         std::getenv("GLS_MG_GRAPH") != nullptr;
}
// everything the captured launches bake in: the level's OpParams (pointers, time coefficients,
// viscosity), the sweep count and damping, and the buffers the sweeps read and write. Buffer
// CONTENTS (state, linearization, diagonal) are read at replay time, so a new Newton state with
// unchanged parameters replays the same graph.
std::vector<unsigned char> coarse_graph_key(gls_ctx *g, const double *b, const double *x, const double *y,
                                                   int pre, double om) {
  const gls::OpParams P = make_params(g);
  const void *ptrs[7] = {b, x, y, g->diag.p, g->qdata.p, g->qdata32.p, brick_slab(g)};
  const int64_t ints[5] = {pre, g->n_dofs, (int64_t)g->smooth_f32, (int64_t)slab_f32(), (int64_t)gls::cube_gather_enabled()};
  std::vector<unsigned char> k(sizeof(P) + sizeof(ptrs) + sizeof(ints) + sizeof(om));
  unsigned char *o = k.data();
  std::memcpy(o, &P, sizeof(P));
  std::memcpy(o += sizeof(P), ptrs, sizeof(ptrs));
  std::memcpy(o += sizeof(ptrs), ints, sizeof(ints));
  std::memcpy(o + sizeof(ints), &om, sizeof(om));
  return k;
}
// capture x = csweeps damped-Jacobi sweeps from x = 0 on c's stream; a refused capture leaves the
// plain launches in place (cgraph_failed)
int coarse_graph_capture(gls_ctx *c, gls_ctx *g, const double *b, double *x, double *y, int pre, double om) {
  auto &mg = c->mg;
  hipStream_t s = c->stream;
  GLS_TRY(ensure_diag(g));
  GLS_TRY(g->smooth_f32 ? ensure_qdata32(g, !g->smooth_oseen) : ensure_qdata(g));
  if (g->use_colors && g->acc.n != (size_t)g->n_dofs) GLS_TRY(g->acc.alloc((size_t)g->n_dofs));  // no malloc in capture
  const bool tim = g->timing;
  g->timing = false;  // no event records inside the capture
  hipGraph_t gr = nullptr;
  int rc = GLS_OK;
  hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    if (hipError_t e1 = gls::mg_jacobi_update(x, b, nullptr, g->diag.p, om, g->n_dofs, 1, s); e1 != hipSuccess)
      e = e1;
    for (int it = 1; it < pre && rc == GLS_OK && e == hipSuccess; ++it) rc = smoother_sweep(g, x, b, y, om);
    const hipError_t e2 = hipStreamEndCapture(s, &gr);
    if (e == hipSuccess) e = e2;
  }
  g->timing = tim;
  hipGraphExec_t ex = nullptr;
  if (rc == GLS_OK && e == hipSuccess && gr) e = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
  if (gr) (void)hipGraphDestroy(gr);
  if (rc != GLS_OK || e != hipSuccess || !ex) {
    (void)hipGetLastError();
    if (ex) (void)hipGraphExecDestroy(ex);
    mg.cgraph_failed = true;
    if (std::getenv("GLS_MG_VERBOSE")) std::printf("mg: coarse graph capture refused (%s)\n", hipGetErrorString(e));
    return GLS_OK;
  }
  mg.cgraph.h = ex;
  mg.cgraph_key = coarse_graph_key(g, b, x, y, pre, om);
  return GLS_OK;
}

// x = pre smoothing sweeps from x = 0 on level g: its ILU(0) when zs (the scratch) is given, else damped Jacobi;
// residual: then y = b - A x (y is the sweeps' scratch before that). x0_ready: x already holds the first damped-Jacobi
// sweep from 0, stored by the kernel that wrote b (mg_first_producer_ok)
int mg_presmooth(gls_ctx *g, hipStream_t s, int pre, double om, double *zs, const double *b, double *x, double *y,
                 bool residual, bool x0_ready = false) {
  const int64_t n = g->n_dofs;
  if (pre > 0 && zs) {
    GLS_TRY(ensure_ilu(g));
    GLS_TRY(apply_ilu(g, b, x));  // first sweep from x = 0: x = M^-1 b
    for (int it = 1; it < pre; ++it) GLS_TRY(smoother_sweep(g, x, b, y, om, zs));
  } else if (pre > 0 && g->vanka.smooth) {
    GLS_TRY(vanka_sweep(g, x, b, y, om, true));  // first sweep from x = 0: the residual is b
    for (int it = 1; it < pre; ++it) GLS_TRY(smoother_sweep(g, x, b, y, om));
  } else if (pre > 0) {
    if (!x0_ready) HIP_TRY(gls::mg_jacobi_update(x, b, nullptr, g->diag.p, om, n, 1, s));  // first sweep from x = 0
    for (int it = 1; it < pre; ++it) GLS_TRY(smoother_sweep(g, x, b, y, om));
  } else {
    HIP_TRY(gls::vec_fill(x, n, 0.0, s));
  }
  if (!residual) return GLS_OK;
  if (pre > 0) return smoother_apply(g, x, y, b);  // y = b - A x
  HIP_TRY(gls::vec_copy(y, b, n, s));  // x = 0: the residual is b
  return GLS_OK;
}
// Level l's cycle starts with a damped-Jacobi sweep from 0 as a launch of its own (mg_presmooth's update; not the
// exact solve, the replica, the coarse graph, ILU smoothing or the opt-in first_sweep_fusable path), so the kernel
// that writes the level's right-hand side may store x = 0 + omega b / D with it and the cycle skip that launch:
// the same expression on the same operands, bitwise the separate update. GLS_MG_FIRST_PRODUCER=0 (read per call) or
// GLS_MG_NO_FUSE keep the update launches.
bool mg_first_producer_ok(gls_ctx *c, int l) {
  auto &mg = c->mg;
  const int L = (int)mg.lev.size();
  if (l < 0 || l >= L) return false;
  const char *e = std::getenv("GLS_MG_FIRST_PRODUCER");
  if ((e && std::atoi(e) == 0) || std::getenv("GLS_MG_NO_FUSE") != nullptr) return false;
  gls_ctx *g = mg.lev[(size_t)l];
  if (l == L - 1 && (mg.replica || mg.coarse.ok)) return false;
  const int pre = l == L - 1 ? mg.csweeps : mg.lpre[(size_t)l];
  if (pre < 1 || g->dist.on || g->stream != c->stream || g->vanka.smooth) return false;
  if (l == L - 1 && l > 0 && pre > 1 && coarse_graph_eligible(c, g, mgbuf(c, l, MB_B), mgbuf(c, l, MB_X))) return false;
  if (pre == 1 && l < L - 1 && first_sweep_fusable(g)) return false;
  return !(mg.ilu_smooth && g->ilu.on && !g->ilu.probe_only);
}
// the coarsest level's exact solve; the first one of a state waits for the side stream's factorization
int mg_coarse_solve(gls_ctx *c, gls_ctx *g, const double *b, double *x) {
  auto &mg = c->mg;
  if (const int rc = mg.coarse.finish(c->stream); rc < 0) {
    mg.dirty = true;
    return rc;
  }
  return mg.coarse.solve(c->stream, b, x, g->ilu.perm.p);
}
}  // namespace

namespace gls_impl {  // declared in gls_ctx.hpp
// one V-cycle with the replica hierarchy below the distributed fine level (gls_mg_attach_replica)
int mg_vcycle_rep2(gls_ctx *c, const double *b, double *x) {
  auto &mg = c->mg;
  gls_ctx *r = mg.rep2;
  const int64_t n = c->n_dofs, ng = r->n_dofs;
  hipStream_t s = c->stream;
  GLS_TRY(ensure_diag(c));
  double *y = mgbuf(c, 0, MB_Y);
  double *zs = mg.ilu_smooth && c->ilu.on && !c->ilu.probe_only ? mgbuf(c, 0, MB_BOX) : nullptr;
  const int pre = mg.lpre[0], post = mg.lpost[0];
  GLS_TRY(mg_presmooth(c, s, pre, mg.omega, zs, b, x, y, true));
  // restriction: the owned rows' part of P^T y on this rank, summed over ranks
  HIP_TRY(gls::vec_csr_spmv(mg.rep_b.p, y, mg.r2r_off.p, mg.r2r_col.p, mg.r2r_w.p, ng, false, s, mg.r2r_lane));
  GLS_TRY(dist_allreduce_vector(c, mg.rep_b.p, ng));
  HIP_TRY(gls::vec_set_indexed(mg.rep_b.p, r->con_dofs.p, nullptr, (int64_t)r->con_dofs.n, s));
  if (mg.coarse.ok) {  // the replica level is the coarsest: its exact solve, every rank
    GLS_TRY(mg_coarse_solve(c, r, mg.rep_b.p, mg.rep_x.p));
  } else {
    GLS_TRY(gls_apply_preconditioner(r, mg.rep_b.p, mg.rep_x.p));  // the replica's own V-cycle, every rank
  }
  HIP_TRY(gls::vec_csr_spmv(y, mg.rep_x.p, mg.r2p_off.p, mg.r2p_col.p, mg.r2p_w.p, n, false, s, mg.r2p_lane));
  HIP_TRY(gls::vec_set_indexed(y, c->con_dofs.p, nullptr, (int64_t)c->con_dofs.n, s));
  HIP_TRY(gls::vec_axpy(x, 1.0, y, n, s));
  for (int it = 0; it < post; ++it) GLS_TRY(smoother_sweep(c, x, b, y, mg.omega, zs));
  return GLS_OK;
}

// The fine level's cycle may take its first sweep from the kernel that writes its right-hand side (GMRES's
// projection): the plain V-cycle on one rank (not rep2; mg_first_producer_ok covers the rest). *d = nullptr: no
int mg_fine_first_producer(gls_ctx *c, const double **d, double *omega) {
  *d = nullptr;
  auto &mg = c->mg;
  if (!mg.on || mg.rep_csr || mg.lev.empty() || c->dist.on || !mg_first_producer_ok(c, 0)) return GLS_OK;
  gls_ctx *g = mg.lev[0];
  GLS_TRY(ensure_diag(g));
  *d = g->diag.p;
  *omega = mg.lev.size() == 1 ? mg.comega : mg.omega;
  return GLS_OK;
}

// x = V-cycle(b) on level l (x, b are level-l vectors)
int mg_vcycle(gls_ctx *c, int l, const double *b, double *x, bool x0_ready) {
  auto &mg = c->mg;
  const int L = (int)mg.lev.size();
  gls_ctx *g = mg.lev[l];
  GLS_TRY(ensure_diag(g));
  const int64_t n = g->n_dofs;
  double *y = mgbuf(c, l, MB_Y);
  hipStream_t s = c->stream;
  if (l == L - 1 && mg.replica) {  // the replica's cycle on the gathered right-hand side, every rank
    GLS_TRY(replica_gather(c, b, mg.rep_b.p));
    GLS_TRY(gls_apply_preconditioner(mg.replica, mg.rep_b.p, mg.rep_x.p));
    HIP_TRY(gls::vec_pack_dofs(mg.rep_x.p, mg.rep_map.p, n, x, c->stream));
    return GLS_OK;
  }
  if (l == L - 1 && mg.coarse.ok) return mg_coarse_solve(c, g, b, x);  // exact coarsest-level solve
  const int pre = l == L - 1 ? mg.csweeps : mg.lpre[(size_t)l];
  const double om = l == L - 1 ? mg.comega : mg.omega;
  if (l == L - 1 && l > 0 && pre > 1 && coarse_graph_eligible(c, g, b, x)) {
    GLS_TRY(ensure_diag(g));  // contents the replay reads: current for this state
    GLS_TRY(g->smooth_f32 ? ensure_qdata32(g, !g->smooth_oseen) : ensure_qdata(g));
    if (mg.cgraph.h && mg.cgraph_key != coarse_graph_key(g, b, x, y, pre, om)) mg.cgraph.reset();
    if (!mg.cgraph.h) GLS_TRY(coarse_graph_capture(c, g, b, x, y, pre, om));
    if (mg.cgraph.h) {
      HIP_TRY(hipGraphLaunch(mg.cgraph.h, s));
      return GLS_OK;
    }
  }
  // one pre-sweep from 0 on a fused level: x = omega D^-1 b is formed inside the residual's J.v
  const bool first_fused = pre == 1 && l < L - 1 && first_sweep_fusable(g);
  double *zs = mg.ilu_smooth && g->ilu.on && !g->ilu.probe_only ? mgbuf(c, l, MB_BOX) : nullptr;  // ILU smoothing scratch
  // bc = R (b - A x), constrained rows zeroed, in one J.v + one sum (first_fused: x = omega D^-1 b formed there too)
  const bool fused_restrict = l < L - 1 && pre > 0 && mg_fused_restrict_ok(c, l);
  if (!first_fused) GLS_TRY(mg_presmooth(g, s, pre, om, zs, b, x, y, l < L - 1 && !fused_restrict, x0_ready));
  if (l == L - 1) return GLS_OK;
  // residual -> coarse right-hand side: restrict the owned rows, export-add coarse ghost rows
  gls_ctx *h = mg.lev[l + 1];
  double *bc = mgbuf(c, l + 1, MB_B), *xc = mgbuf(c, l + 1, MB_X);
  // the restriction's sum stores level l + 1's first sweep from 0 with its right-hand side
  const bool xc_ready = fused_restrict && mg_first_producer_ok(c, l + 1);
  if (fused_restrict) {
    GLS_TRY(mg_residual_restrict_fused(c, l, x, b, bc, first_fused ? om : 0.0, xc_ready ? xc : nullptr,
                                       l + 1 == L - 1 ? mg.comega : mg.omega));
  } else {
    if (first_fused) GLS_TRY(jacobian_apply_f32(g, x, y, b, om, g->smooth_oseen));  // x = omega D^-1 b, y = b - A x
    GLS_TRY(mg_restrict(c, l, y, bc));
    HIP_TRY(gls::vec_set_indexed(bc, h->con_dofs.p, nullptr, (int64_t)h->con_dofs.n, s));
  }
  GLS_TRY(mg_vcycle(c, l + 1, bc, xc, xc_ready));
  // prolongate the coarse correction (ghost values imported first). x += P xc in the transfer's
  // store on one rank: the coarse correction vanishes on the coarse Dirichlet rows (zero rhs rows,
  // D_c-scaled sweeps) and the nested Qk interpolation maps them onto the fine Dirichlet rows, so
  // P xc is exactly 0 there, as the zeroing below makes it in the general path
  const bool pro = mg_fused_prolong_ok(c, l);  // x += P xc inside the first post-sweep's J.v and slab sum
  if (pro) {  // nothing here: the sweep below gathers x + P xc
  } else if (mg_prolong_add_ok(c, l)) {
    GLS_TRY(mg_prolong(c, l, xc, x, true));
  } else {
    GLS_TRY(mg_prolong(c, l, xc, y));
    HIP_TRY(gls::vec_set_indexed(y, g->con_dofs.p, nullptr, (int64_t)g->con_dofs.n, s));
    HIP_TRY(gls::vec_axpy(x, 1.0, y, n, s));
  }
  for (int it = 0; it < mg.lpost[(size_t)l]; ++it)
    GLS_TRY(smoother_sweep(g, x, b, y, mg.omega, zs, pro && it == 0 ? xc : nullptr));
  return GLS_OK;
}
}  // namespace gls_impl

extern "C" {

int gls_mg_transfer(gls_ctx *c, int level, int direction, const double *in, double *out) {
  GLS_TRY(check_ctx(c));
  auto &mg = c->mg;
  if (!mg.on) return set_err(GLS_EINVAL, "gls_mg_transfer: no multigrid attached");
  if (level < 0 || level + 1 >= (int)mg.lev.size() || (direction != 0 && direction != 1) || !in || !out || in == out)
    return set_err(GLS_EINVAL, "gls_mg_transfer: bad level / direction / pointers");
  if (direction == 0) return mg_restrict(c, level, in, out);
  double *xc = mgbuf(c, level + 1, MB_X);  // ghost import writes into the coarse vector: work on a copy
  HIP_TRY(gls::vec_copy(xc, in, mg.lev[(size_t)level + 1]->n_dofs, c->stream));
  return mg_prolong(c, level, xc, out);
}

int gls_mg_residual_restrict(gls_ctx *c, int level, const double *x, const double *b, double *bc, int *fused) {
  GLS_TRY(check_ctx(c));
  auto &mg = c->mg;
  if (!mg.on) return set_err(GLS_EINVAL, "gls_mg_residual_restrict: no multigrid attached");
  if (level < 0 || level + 1 >= (int)mg.lev.size() || !x || !b || !bc)
    return set_err(GLS_EINVAL, "gls_mg_residual_restrict: bad level / pointers");
  GLS_TRY(mg_prepare(c));  // the levels' states, as the V-cycle sees them
  const bool f = mg_fused_restrict_ok(c, level);
  if (fused) *fused = f ? 1 : 0;
  if (f) return mg_residual_restrict_fused(c, level, const_cast<double *>(x), b, bc);
  gls_ctx *g = mg.lev[(size_t)level], *h = mg.lev[(size_t)level + 1];
  double *y = mgbuf(c, level, MB_Y);
  GLS_TRY(smoother_apply(g, x, y, b));
  GLS_TRY(mg_restrict(c, level, y, bc));
  HIP_TRY(gls::vec_set_indexed(bc, h->con_dofs.p, nullptr, (int64_t)h->con_dofs.n, c->stream));
  return GLS_OK;
}

int gls_mg_prolong_smooth(gls_ctx *c, int level, const double *xc, double *x, const double *b, double omega, int *fused) {
  GLS_TRY(check_ctx(c));
  auto &mg = c->mg;
  if (!mg.on) return set_err(GLS_EINVAL, "gls_mg_prolong_smooth: no multigrid attached");
  if (level < 0 || level + 1 >= (int)mg.lev.size() || !xc || !x || !b || x == b || omega < 0.0)
    return set_err(GLS_EINVAL, "gls_mg_prolong_smooth: bad level / pointers / omega");
  GLS_TRY(mg_prepare(c));  // the levels' states, as the V-cycle sees them
  gls_ctx *g = mg.lev[(size_t)level];
  const bool f = mg_fused_prolong_ok(c, level);
  if (fused) *fused = f ? 1 : 0;
  double *y = mgbuf(c, level, MB_Y);
  double *zs = mg.ilu_smooth && g->ilu.on && !g->ilu.probe_only ? mgbuf(c, level, MB_BOX) : nullptr;
  double *xcw = mgbuf(c, level + 1, MB_X);  // the V-cycle's coarse vector (ghost import writes into it): a copy
  if (xcw != xc) HIP_TRY(gls::vec_copy(xcw, xc, mg.lev[(size_t)level + 1]->n_dofs, c->stream));
  if (f) return smoother_sweep(g, x, b, y, omega, zs, xcw);
  if (mg_prolong_add_ok(c, level)) {
    GLS_TRY(mg_prolong(c, level, xcw, x, true));
  } else {
    GLS_TRY(mg_prolong(c, level, xcw, y));
    HIP_TRY(gls::vec_set_indexed(y, g->con_dofs.p, nullptr, (int64_t)g->con_dofs.n, c->stream));
    HIP_TRY(gls::vec_axpy(x, 1.0, y, g->n_dofs, c->stream));
  }
  return smoother_sweep(g, x, b, y, omega, zs);
}


int gls_set_lattice(gls_ctx *c, int n1d, const int64_t *l2g) {
  GLS_TRY(check_ctx(c));
  if (c->dim != 3 || n1d < 2 || !l2g) return set_err(GLS_EINVAL, "gls_set_lattice: 3D, n1d >= 2, map required");
  int lo[3] = {n1d, n1d, n1d}, hi[3] = {-1, -1, -1};
  for (int i = 0; i < c->n_vnodes; ++i) {
    const int64_t g = l2g[i];
    if (g < 0 || g >= (int64_t)n1d * n1d * n1d) return set_err(GLS_EINVAL, "lattice node out of range");
    const int x[3] = {(int)(g % n1d), (int)((g / n1d) % n1d), (int)(g / ((int64_t)n1d * n1d))};
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], x[a]); hi[a] = std::max(hi[a], x[a]); }
  }
  int bd[3];
  for (int a = 0; a < 3; ++a) bd[a] = hi[a] - lo[a] + 1;
  const int64_t nbox = (int64_t)bd[0] * bd[1] * bd[2];
  if (nbox != c->n_vnodes) return set_err(GLS_EINVAL, "local nodes do not fill a box (%lld != %d)", (long long)nbox, c->n_vnodes);
  std::vector<int32_t> map((size_t)nbox, -1);
  for (int i = 0; i < c->n_vnodes; ++i) {
    const int64_t g = l2g[i];
    const int64_t x = g % n1d - lo[0], y = (g / n1d) % n1d - lo[1], z = g / ((int64_t)n1d * n1d) - lo[2];
    int32_t &m = map[(size_t)((z * bd[1] + y) * bd[0] + x)];
    if (m >= 0) return set_err(GLS_EINVAL, "duplicate lattice node");
    m = i;
  }
  GLS_TRY(c->lat.map.upload(map.data(), map.size()));
  c->lat.n1d = n1d;
  for (int a = 0; a < 3; ++a) { c->lat.box0[a] = lo[a]; c->lat.bdim[a] = bd[a]; }
  c->lat.set = true;
  return GLS_OK;
}

// the sweep parameters, level buffers and the coarsest-level direct solve of an attached hierarchy
static int mg_attach_common(gls_ctx *c, const gls_mg_params *p) {
  auto &mg = c->mg;
  mg.k = c->k;
  mg.pre = p->pre_smooth > 0 ? p->pre_smooth : (p->pre_smooth < 0 ? 0 : 2);
  mg.post = p->post_smooth >= 0 ? p->post_smooth : 2;
  mg.csweeps = p->coarse_sweeps > 0 ? p->coarse_sweeps : 30;
  mg.omega = p->omega > 0 ? p->omega : (p->smoother == 3 ? 0.8 : 0.6);  // cell-Vanka: the best V(1,1) damping
  mg.comega = p->coarse_omega > 0 ? p->coarse_omega : (p->smoother == 3 ? 0.6 : mg.omega);  // coarsest: Jacobi sweeps
  mg.lpre.assign((size_t)p->n_levels, mg.pre);
  mg.lpost.assign((size_t)p->n_levels, mg.post);
  if (p->level_sweeps)
    for (int l = 0; l < p->n_levels; ++l) {
      if (p->level_sweeps[2 * l] < 0 || p->level_sweeps[2 * l + 1] < 0) return set_err(GLS_EINVAL, "mg: negative level sweeps");
      mg.lpre[(size_t)l] = p->level_sweeps[2 * l];
      mg.lpost[(size_t)l] = p->level_sweeps[2 * l + 1];
    }
  for (auto *g : mg.lev) g->smooth_f32 = p->mixed_precision != 0;
  // the smoother's operator: Newton's Jacobian, or its Oseen (Picard) part (FP32 brick levels only: the
  // pencil J.v drops the (grad u) v terms)
  {
    const bool os = p->smoother_operator == 1;
    if (p->smoother_operator < 0 || p->smoother_operator > 1) return set_err(GLS_EINVAL, "mg: smoother_operator 0 or 1");
    for (auto *g : mg.lev) g->smooth_oseen = os && g->smooth_f32;
  }
  mg.ilu_smooth = p->smoother == 1 || p->smoother == 2;
  if (p->smoother < 0 || p->smoother > 3 || ((mg.ilu_smooth || p->smoother == 3) && !mg.csr))
    return set_err(GLS_EINVAL, "mg: smoother 0 (Jacobi), 1 (ILU), 2 (ILU below the finest level) or 3 (cell-Vanka); 1 - 3 on "
                               "gls_mg_attach_transfers hierarchies");
  for (int l = 0; l < p->n_levels; ++l)
    for (int b = 0; b < MB_N; ++b) {
      mg.bufs.emplace_back(new DevBuf<double>());
      const bool need = b == MB_BOX ? (mg.boxed || mg.ilu_smooth) : (l > 0 || b == MB_Y);
      if (need)
        GLS_TRY(mg.bufs.back()->alloc(b == MB_BOX && mg.boxed ? (size_t)(4 * mg_nbox(c, l)) : (size_t)mg.lev[l]->n_dofs));
    }
  if (mg.ilu_smooth)  // ILU(0) on every level above the coarsest (multicolor order); smoother 2: not the finest
    for (int l = p->smoother == 2 ? 1 : 0; l + 1 < p->n_levels; ++l) {
      gls_ctx *g = mg.lev[(size_t)l];
      // multicolor order on every level. As a smoother the color-by-color ILU(0) is both faster per sweep (no level-scheduled csrsv) and
      // stronger: configs[3] --precond hmg 38 -> 26 GMRES iterations, 3.97 -> 1.37 s wall, the linear solves
      // 1.72 -> 0.08 s (profiles/r05_app_configs3_hmg_ilu_order.txt)
      GLS_TRY(gls_ilu_set_options(g, GLS_ILU_ORDER_MULTICOLOR, 0));
      GLS_TRY(gls_ilu_attach(g, 0, 1e-12, 1.0));
      mg.ilu_levels.push_back(g);  // detached again by gls_mg_detach
    }
  if (p->smoother == 3)  // additive cell-Vanka on every level above the coarsest: the maps now, the inverses per state
    for (int l = 0; l + 1 < p->n_levels; ++l) {
      gls_ctx *g = mg.lev[(size_t)l];
      GLS_TRY(vanka_attach(g));
      g->vanka.smooth = true;
    }
  // direct coarsest solve: single GPU; dense arrays up to kDirectMax DoFs (FP64 LU up to kDirectSmall, FP32 above), band
  // storage beyond or when asked (coarse_direct 2)
  {
    const int64_t nco = mg.lev.back()->n_dofs;
    const int want = p->coarse_direct;
    if (want > 2) return set_err(GLS_EINVAL, "mg: coarse_direct -1, 0, 1 or 2");
    if (want > 0 && mg.boxed) return set_err(GLS_EINVAL, "mg: direct coarse solve needs one GPU");
    mg.direct = want > 0 || (want == 0 && !mg.boxed && nco <= 2048);
    // 1 up to kDirectMax: the dense routes; above, or 2: band storage (the callers ran band_precheck first)
    if (mg.direct) {
      const bool band = band_route_wanted(p, mg.lev.back());
      const int rc = mg_coarse_setup("mg", c, mg.lev.back(), band);
      // the exact byte check needs the probing ILU, attached after the detach: its refusal leaves nothing half
      // attached (the smoother ILUs and Vanka maps put on the levels above go again; the message stays)
      if (rc < 0 && band) (void)gls_mg_detach(c);
      GLS_TRY(rc);
    }
  }
  mg.on = true;
  mg.dirty = true;
  // one stream for the whole V-cycle: the coarse levels' kernels are ordered with the transfers
  for (size_t l = 1; l < mg.lev.size(); ++l)
    if (mg.lev[l]->stream != c->stream) GLS_TRY(gls_set_stream(mg.lev[l], c->stream));
  return GLS_OK;
}

namespace {
// nodes per direction of the Qk lattice of a box of n[a] cells: a periodic axis has no node of its own at the far face
std::array<int, 3> wrapped_dims(const std::array<int, 3> &n, int K, int mask) {
  std::array<int, 3> d;
  for (int a = 0; a < 3; ++a) d[a] = K * n[a] + (((mask >> a) & 1) ? 0 : 1);
  return d;
}
// level g's cells against the lexicographic wrapped lattice dm of n[0] x n[1] x n[2] cells (the numbering of
// gls_mesh_hyper_cube and gls_mesh_hyper_rectangle with this mask),
// cell by cell and in any cell order: a cell's first node fixes its origin, a multiple of K per axis, every other node
// follows modulo the lattice, and no origin is taken twice. nullptr, or what differs
const char *wrapped_lattice_mismatch(const gls_ctx *g, const std::array<int, 3> &n, int K, const std::array<int, 3> &dm,
                                     std::vector<int32_t> &cv) {
  const int K1 = K + 1, N3 = K1 * K1 * K1;
  if ((int64_t)n[0] * n[1] * n[2] != g->n_cells || (int64_t)dm[0] * dm[1] * dm[2] != g->n_vnodes) return "cell or node count";
  if (g->cell_vnodes.n != (size_t)g->n_cells * N3) return "cell node array";
  cv.resize(g->cell_vnodes.n);
  if (hipMemcpy(cv.data(), g->cell_vnodes.p, sizeof(int32_t) * cv.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return "cell node array could not be read";
  std::vector<uint8_t> seen((size_t)g->n_cells, 0);
  for (int64_t cl = 0; cl < g->n_cells; ++cl) {
    const int32_t *v = cv.data() + (size_t)cl * N3;
    if (v[0] < 0 || v[0] >= g->n_vnodes) return "node out of range";
    const int o[3] = {v[0] % dm[0], (v[0] / dm[0]) % dm[1], v[0] / (dm[0] * dm[1])};
    for (int a = 0; a < 3; ++a)
      if (o[a] % K != 0 || o[a] / K >= n[a]) return "cell origin off the lattice";
    uint8_t &sn = seen[(size_t)(((int64_t)(o[2] / K) * n[1] + o[1] / K) * n[0] + o[0] / K)];
    if (sn) return "two cells at one origin";
    sn = 1;
    for (int e = 1; e < N3; ++e) {
      const int64_t x = (o[0] + e % K1) % dm[0], y = (o[1] + (e / K1) % K1) % dm[1], z = (o[2] + e / (K1 * K1)) % dm[2];
      if (v[e] != (int32_t)(x + dm[0] * (y + dm[1] * z))) return "cell nodes";
    }
  }
  return nullptr;
}

// gls_mg_attach (mask 0), gls_mg_attach_periodic and gls_mg_attach_box (cells != nullptr: level l has cells[a] >> l
// cells on axis a instead of cbrt(n_cells), and every level is checked against its lattice, mask 0 included)
int mg_attach_nested(gls_ctx *c, const gls_mg_params *p, int mask, const int *cells = nullptr) {
  GLS_TRY(check_ctx(c));
  if (!p || p->n_levels < 2 || !p->levels || p->levels[0] != c) return set_err(GLS_EINVAL, "mg: levels[0] must be ctx");
  if (p->smoother == 3)
    return set_err(GLS_EINVAL, "mg: the cell-Vanka smoother (3) needs a gls_mg_attach_transfers hierarchy of per-cell "
                               "contexts, not the nested brick (pencil) levels");
  if (c->dim != 3 || c->k > 2 || c->k != c->kp) return set_err(GLS_EINVAL, "mg: 3D Q1-Q1 / Q2-Q2 only");
  if (c->hang.on) return set_err(GLS_EINVAL, "mg: not with hanging-node constraints");
  if (c->map_degree > 0) return set_err(GLS_EINVAL, "mg: nested hyper_cube levels only (not mapped cells)");
  // periodic lattices: every level is checked here, before anything is detached (the context keeps what it had)
  std::vector<std::array<int, 3>> pdims;
  if (cells) {
    if (mask < 0 || mask > 7) return set_err(GLS_EINVAL, "mg: periodic_mask has bits 0 - 2 (x, y, z)");
    if (c->dist.on) return set_err(GLS_EINVAL, "mg: box levels run on one rank (the context is distributed)");
    std::vector<int32_t> cv;
    for (int l = 0; l < p->n_levels; ++l) {
      const gls_ctx *g = p->levels[l];
      if (!g || g->dim != 3 || g->k != c->k || g->kp != c->kp)
        return set_err(GLS_EINVAL, "mg level %d: order differs from level 0", l);
      if (g->dist.on) return set_err(GLS_EINVAL, "mg level %d: box levels run on one rank (the level is distributed)", l);
      if (g->hang.on || g->map_degree > 0) return set_err(GLS_EINVAL, "mg level %d: hanging nodes or mapped cells", l);
      std::array<int, 3> n;
      for (int a = 0; a < 3; ++a) {
        const bool per = (mask >> a) & 1;
        if (cells[a] <= 0 || (cells[a] >> l) << l != cells[a])
          return set_err(GLS_EINVAL, "mg level %d axis %d: %d cells do not halve %d times", l, a, cells[a], l);
        n[a] = cells[a] >> l;
        if (n[a] % 2 != 0) return set_err(GLS_EINVAL, "mg level %d axis %d: an odd cell count (%d)", l, a, n[a]);
        if (n[a] < (per ? 4 : 2))
          return set_err(GLS_EINVAL, "mg level %d axis %d: %s axis needs at least %d cells (it has %d)", l, a,
                         per ? "a periodic" : "an open", per ? 4 : 2, n[a]);
      }
      if ((int64_t)n[0] * n[1] * n[2] != g->n_cells)
        return set_err(GLS_EINVAL, "mg level %d not nested (%d cells, %d x %d x %d expected)", l, g->n_cells, n[0], n[1], n[2]);
      const auto dm = wrapped_dims(n, c->k, mask);
      if (const char *why = wrapped_lattice_mismatch(g, n, c->k, dm, cv))
        return set_err(GLS_EINVAL, "mg level %d: its node numbering is not the wrapped lexicographic lattice of the %d x %d x "
                                   "%d box with periodic mask %d (%s)", l, n[0], n[1], n[2], mask, why);
      pdims.push_back(dm);
    }
  } else if (mask) {
    if (mask < 0 || mask > 7) return set_err(GLS_EINVAL, "mg: periodic_mask has bits 0 - 2 (x, y, z)");
    if (c->dist.on)
      return set_err(GLS_EINVAL, "mg: periodic nested levels run on one rank (periodic_mask %d on a distributed context)", mask);
    std::vector<int32_t> cv;
    int nprev = 0;
    for (int l = 0; l < p->n_levels; ++l) {
      const gls_ctx *g = p->levels[l];
      if (!g || g->dim != 3 || g->k != c->k || g->kp != c->kp)
        return set_err(GLS_EINVAL, "mg level %d: order differs from level 0", l);
      if (g->dist.on) return set_err(GLS_EINVAL, "mg level %d: periodic nested levels run on one rank (the level is distributed)", l);
      if (g->hang.on || g->map_degree > 0) return set_err(GLS_EINVAL, "mg level %d: hanging nodes or mapped cells", l);
      const int n = (int)std::lround(std::cbrt((double)g->n_cells));
      if (n < 2) return set_err(GLS_EINVAL, "mg level %d: a periodic direction needs at least 2 cells (it has %d)", l, n);
      if (l > 0 && nprev != 2 * n) return set_err(GLS_EINVAL, "mg level %d not nested (%d cells per direction below %d)", l, n, nprev);
      const auto dm = wrapped_dims({n, n, n}, c->k, mask);
      if (const char *why = wrapped_lattice_mismatch(g, {n, n, n}, c->k, dm, cv))
        return set_err(GLS_EINVAL, "mg level %d: its node numbering is not the wrapped lexicographic lattice of the "
                                   "hyper_cube with periodic mask %d (%s)", l, mask, why);
      pdims.push_back(dm);
      nprev = n;
    }
  }
  GLS_TRY(band_precheck("mg", c, p, p->levels[p->n_levels - 1]));  // refused before anything is detached
  GLS_TRY(gls_mg_detach(c));  // a previous attach's levels / smoother ILUs
  auto &mg = c->mg;
  mg.boxed = c->dist.on;
  for (int l = 0; l < p->n_levels; ++l) {
    gls_ctx *g = p->levels[l];
    if (!g || g->dim != 3 || g->k != c->k || g->kp != c->kp || g->dist.on != mg.boxed)
      return set_err(GLS_EINVAL, "mg level %d: order / distribution differs from level 0", l);
    std::array<int, 3> dm;
    if (!pdims.empty()) {
      dm = pdims[(size_t)l];
    } else if (mg.boxed) {
      if (!g->lat.set) return set_err(GLS_EINVAL, "mg level %d: distributed level without gls_set_lattice", l);
      for (int a = 0; a < 3; ++a) dm[a] = g->lat.bdim[a];
      if (l > 0) {
        const gls_ctx *f = p->levels[l - 1];
        if (f->lat.n1d != 2 * g->lat.n1d - 1) return set_err(GLS_EINVAL, "mg level %d not nested", l);
        for (int a = 0; a < 3; ++a)
          if (f->lat.box0[a] != 2 * g->lat.box0[a] || f->lat.bdim[a] != 2 * g->lat.bdim[a] - 1)
            return set_err(GLS_EINVAL, "mg level %d: partition not nested (rank box %d)", l, a);
      }
    } else {
      const int n = (int)std::lround(std::cbrt((double)g->n_vnodes));
      if ((int64_t)n * n * n != g->n_vnodes) return set_err(GLS_EINVAL, "mg level %d is not an n^3 lattice", l);
      if (l > 0 && mg.dims.back()[0] != 2 * n - 1) return set_err(GLS_EINVAL, "mg level %d not nested", l);
      dm = {n, n, n};
    }
    mg.lev.push_back(g);
    mg.dims.push_back(dm);
  }
  // 1D transfer taps: fine lattice index i sits at x = i / (2k) coarse cells from the box origin;
  // prolongation interpolates the coarse Qk field of the parent cell (equidistant nodes, k <= 2).
  // A periodic axis (nf = 2 nc): the parent cell is floor(x) without the clamp and coarse node cc k + q wraps modulo
  // nc. The tables hold the indices unwrapped (the prolongation's nc for node 0 behind the last cell, the
  // restriction's i - nf for the fine nodes before node 0), ascending per output, and the kernels wrap where they load.
  const int K = c->k;
  size_t xwork = 0;
  for (int l = 0; l + 1 < p->n_levels; ++l) {
    std::unique_ptr<gls_ctx::MG::Taps> T(new gls_ctx::MG::Taps);
    T->two_pass = true;
    // the fused transfers' closed form is the open cube's (nf = 2 nc - 1, Morton bricks)
    T->q2_brick = K == 2 && mask == 0 && (!cells || (cells[0] == cells[1] && cells[1] == cells[2]));
    T->wrap = mask != 0;
    xwork =std::max(xwork, (size_t)4 * mg.dims[l + 1][0] * mg.dims[l + 1][1] * mg.dims[l][2]);
    for (int a = 0; a < 3; ++a) {
      const bool per = (mask >> a) & 1;
      const int nf = mg.dims[l][a], nc = mg.dims[l + 1][a], ncc = (nf - 1) / (2 * K);
      if (per ? nf != 2 * nc : nf != 2 * nc - 1) return set_err(GLS_EINVAL, "mg level %d not nested (axis %d)", l + 1, a);
      std::vector<int32_t> pi((size_t)nf * 5, 0), ri((size_t)nc * 5, 0);
      std::vector<double> pw((size_t)nf * 5, 0.0), rw((size_t)nc * 5, 0.0);
      std::vector<int32_t> rn((size_t)nc, 0), pn((size_t)nf, 0);
      for (int i = 0; i < nf; ++i) {
        const double x = (double)i / (2.0 * K);
        const int cc = per ? (int)std::floor(x) : std::min((int)std::floor(x), ncc - 1);
        const double xi = x - cc;
        int np = 0;
        for (int q = 0; q <= K; ++q) {
          double L = 1.0;
          for (int b = 0; b <= K; ++b)
            if (b != q) L *= (xi * K - b) / (double)(q - b);
          if (L == 0.0) continue;
          const int ju = cc * K + q, j = per ? ju % nc : ju;  // ju == nc: coarse node 0 behind the seam
          pi[(size_t)i * 5 + np] = ju;
          pw[(size_t)i * 5 + np] = L;
          ++np;
          if (rn[(size_t)j] >= 5) return set_err(GLS_EINVAL, "mg: restriction stencil wider than 5");
          ri[(size_t)j * 5 + rn[(size_t)j]] = ju != j ? i - nf : i;
          rw[(size_t)j * 5 + rn[(size_t)j]] = L;
          ++rn[(size_t)j];
        }
        pn[(size_t)i] = np;
        if (K == 2 && !per) {  // the closed form of the in-kernel restriction, checked tap by tap
          static const double W[5][3] = {{1, 0, 0}, {0.375, 0.75, -0.125}, {0, 1, 0}, {-0.125, 0.75, 0.375}, {0, 0, 1}};
          const int m = i - 4 * cc;
          int nz = 0;
          for (int q = 0; q < 3; ++q) nz += W[m][q] != 0.0;
          bool same = np == nz;
          for (int e = 0; same && e < np; ++e) {
            const int q = pi[(size_t)i * 5 + e] - 2 * cc;
            same = q >= 0 && q < 3 && pw[(size_t)i * 5 + e] == W[m][q];
          }
          T->q2_brick = T->q2_brick && same && nf == 2 * nc - 1;
        }
      }
      if (per)  // the seam's rows took their taps before node 0 last: ascending order again
        for (int j = 0; j < nc; ++j)
          for (int e = 1; e < rn[(size_t)j]; ++e)
            for (int f = e; f > 0 && ri[(size_t)j * 5 + f] < ri[(size_t)j * 5 + f - 1]; --f) {
              std::swap(ri[(size_t)j * 5 + f], ri[(size_t)j * 5 + f - 1]);
              std::swap(rw[(size_t)j * 5 + f], rw[(size_t)j * 5 + f - 1]);
            }
      if (a < 2)
        T->two_pass = T->two_pass && gls::mg_transfer_tile_fits(0, a, nf, pi.data(), pn.data()) &&
                      gls::mg_transfer_tile_fits(1, a, nc, ri.data(), rn.data());
      GLS_TRY(T->pi[a].upload(pi.data(), pi.size()));
      GLS_TRY(T->pw[a].upload(pw.data(), pw.size()));
      GLS_TRY(T->ri[a].upload(ri.data(), ri.size()));
      GLS_TRY(T->rw[a].upload(rw.data(), rw.size()));
      GLS_TRY(T->pc[a].upload(pn.data(), pn.size()));
      GLS_TRY(T->rc[a].upload(rn.data(), rn.size()));
    }
    // only the two-pass kernels wrap: the one-pass gather would read the unwrapped taps as they stand
    if (T->wrap && !T->two_pass) {
      (void)gls_mg_detach(c);
      return set_err(GLS_EINVAL, "mg level %d: the periodic lattice's taps do not fit the two-pass transfer tiles", l);
    }
    mg.taps.push_back(std::move(T));
  }
  if (xwork) GLS_TRY(mg.xwork.alloc(xwork));
  return mg_attach_common(c, p);
}
}  // namespace

int gls_mg_attach(gls_ctx *c, const gls_mg_params *p) { return mg_attach_nested(c, p, 0); }

int gls_mg_attach_periodic(gls_ctx *c, const gls_mg_params *p, int periodic_mask) {
  return mg_attach_nested(c, p, periodic_mask);
}

int gls_mg_attach_box(gls_ctx *c, const gls_mg_params *p, const int cells[3], int periodic_mask) {
  if (!cells) return set_err(GLS_EINVAL, "gls_mg_attach_box: cells is null");
  return mg_attach_nested(c, p, periodic_mask, cells);
}

int gls_mg_attach_transfers(gls_ctx *c, const gls_mg_params *p, const int64_t *const *p_off, const int32_t *const *p_col,
                            const double *const *p_w, const int64_t *const *inject) {
  GLS_TRY(check_ctx(c));
  if (!p || p->n_levels < 2 || !p->levels || p->levels[0] != c) return set_err(GLS_EINVAL, "mg: levels[0] must be ctx");
  if (!p_off || !p_col || !p_w || !inject) return set_err(GLS_EINVAL, "mg: transfer arrays missing");
  GLS_TRY(band_precheck("mg", c, p, p->levels[p->n_levels - 1]));  // refused before anything is built or detached
  if (p->smoother == 3) {  // refused before anything is detached: the context keeps what it had
    for (int l = 0; l + 1 < p->n_levels; ++l) {
      if (!p->levels[l]) return set_err(GLS_EINVAL, "mg level %d: null", l);
      if (const char *why = vanka_refusal(p->levels[l])) return set_err(GLS_EINVAL, "mg level %d: %s", l, why);
    }
    // the maps too (they refuse a cell that holds a node twice); a refusal drops the maps built here
    std::vector<gls_ctx *> built;
    for (int l = 0; l + 1 < p->n_levels; ++l) {
      gls_ctx *g = p->levels[l];
      if (g->vanka.on) continue;
      const int rc = vanka_attach(g);
      if (rc < 0) {
        for (auto *b : built) b->vanka = gls_ctx::Vanka();
        return rc;
      }
      built.push_back(g);
    }
  }

  GLS_TRY(gls_mg_detach(c));  // a previous attach's levels / smoother ILUs
  auto &mg = c->mg;
  mg.csr = true;
  for (int l = 0; l < p->n_levels; ++l) {
    gls_ctx *g = p->levels[l];
    // the levels may differ in degree (h-p hierarchies: the CSR transfers carry the p-level pairs of
    // gls_fe_space_mg_transfer), not in dimension
    if (!g || g->dim != c->dim || g->dist.on)
      return set_err(GLS_EINVAL, "mg level %d: dimension differs from level 0, or distributed", l);
    mg.lev.push_back(g);
    mg.dims.push_back({0, 0, 0});
  }
  for (int l = 0; l + 1 < p->n_levels; ++l) {
    const int64_t nf = mg.lev[(size_t)l]->n_dofs, nc = mg.lev[(size_t)l + 1]->n_dofs;
    const int64_t *off = p_off[l];
    if (!off || !p_col[l] || !p_w[l] || !inject[l] || off[0] != 0) return set_err(GLS_EINVAL, "mg transfer %d: arrays", l);
    for (int64_t i = 0; i < nf; ++i)
      if (off[i + 1] < off[i]) return set_err(GLS_EINVAL, "mg transfer %d: offsets not monotone", l);
    const int64_t nnz = off[nf];
    std::vector<int64_t> rcnt((size_t)nc + 1, 0);
    for (int64_t j = 0; j < nnz; ++j) {
      if (p_col[l][j] < 0 || p_col[l][j] >= nc) return set_err(GLS_EINVAL, "mg transfer %d: column out of range", l);
      ++rcnt[(size_t)p_col[l][j] + 1];
    }
    for (int64_t j = 0; j < nc; ++j) rcnt[(size_t)j + 1] += rcnt[(size_t)j];
    // R = P^T, each coarse row's terms in ascending fine row order (deterministic sums)
    std::vector<int32_t> rcol((size_t)nnz);
    std::vector<double> rw((size_t)nnz);
    std::vector<int64_t> fill(rcnt.begin(), rcnt.end() - 1);
    for (int64_t i = 0; i < nf; ++i)
      for (int64_t j = off[i]; j < off[i + 1]; ++j) {
        const int64_t slot = fill[(size_t)p_col[l][j]]++;
        rcol[(size_t)slot] = (int32_t)i;
        rw[(size_t)slot] = p_w[l][j];
      }
    std::vector<int32_t> inj((size_t)nc);
    for (int64_t j = 0; j < nc; ++j) {
      if (inject[l][j] < 0 || inject[l][j] >= nf) return set_err(GLS_EINVAL, "mg transfer %d: injection out of range", l);
      inj[(size_t)j] = (int32_t)inject[l][j];
    }
    std::unique_ptr<gls_ctx::MG::Csr> X(new gls_ctx::MG::Csr);
    X->nf = nf;
    X->nc = nc;
    auto lanes = [](double mean) {  // ~2 entries per lane
      int L = 1;
      while (L < 16 && 2.0 * L < mean) L *= 2;
      return L;
    };
    X->plane = lanes((double)nnz / (double)std::max<int64_t>(nf, 1));
    X->rlane = lanes((double)nnz / (double)std::max<int64_t>(nc, 1));
    GLS_TRY(X->poff.upload(off, (size_t)nf + 1));
    GLS_TRY(X->pcol.upload(p_col[l], (size_t)std::max<int64_t>(nnz, 1)));
    GLS_TRY(X->pw.upload(p_w[l], (size_t)std::max<int64_t>(nnz, 1)));
    GLS_TRY(X->roff.upload(rcnt.data(), rcnt.size()));
    GLS_TRY(X->rcol.upload(rcol.data(), std::max<size_t>(rcol.size(), 1)));
    GLS_TRY(X->rw.upload(rw.data(), std::max<size_t>(rw.size(), 1)));
    GLS_TRY(X->inj.upload(inj.data(), inj.size()));
    mg.xfer.push_back(std::move(X));
  }
  return mg_attach_common(c, p);
}

int gls_mg_set_coarse_replica(gls_ctx *c, gls_ctx *replica, int64_t n_local, const int64_t *local_to_replica) {
  GLS_TRY(check_ctx(c));
  auto &mg = c->mg;
  if (!mg.on || mg.lev.size() < 2) return set_err(GLS_EINVAL, "coarse replica: attach the multigrid hierarchy first");
  gls_ctx *g = mg.lev.back();
  if (!replica || replica == c || replica->dist.on) return set_err(GLS_EINVAL, "coarse replica: a single-rank context");
  if (!g->dist.on) return set_err(GLS_EINVAL, "coarse replica: the coarsest level is not distributed");
  if (n_local != g->n_dofs || !local_to_replica) return set_err(GLS_EINVAL, "coarse replica: map of %lld rows expected",
                                                                (long long)g->n_dofs);
  const int64_t ng = replica->n_dofs;
  if (ng >= INT32_MAX) return set_err(GLS_EINVAL, "coarse replica too large");
  std::vector<int32_t> all((size_t)n_local), own_l, own_g;
  const int64_t dv = (int64_t)g->dim * g->n_vnodes;
  for (int64_t i = 0; i < n_local; ++i) {
    const int64_t t = local_to_replica[i];
    if (t < 0 || t >= ng) return set_err(GLS_EINVAL, "coarse replica: row %lld maps outside", (long long)i);
    all[(size_t)i] = (int32_t)t;
    const bool owned = i < dv ? i < (int64_t)g->dim * g->dist.n_owned : i - dv < g->dist.n_owned_p;
    if (owned) {
      own_l.push_back((int32_t)i);
      own_g.push_back((int32_t)t);
    }
  }
  GLS_TRY(mg.rep_map.upload(all.data(), all.size()));
  GLS_TRY(mg.rep_own_loc.upload(own_l.data(), own_l.size()));
  GLS_TRY(mg.rep_own_glob.upload(own_g.data(), own_g.size()));
  GLS_TRY(mg.rep_b.alloc((size_t)ng));
  GLS_TRY(mg.rep_x.alloc((size_t)ng));
  GLS_TRY(mg.rep_tmp.alloc(std::max<size_t>(own_l.size(), 1)));
  for (auto &u : mg.rep_u) GLS_TRY(u.alloc((size_t)ng));
  if (replica->stream != c->stream) GLS_TRY(gls_set_stream(replica, c->stream));
  mg.replica = replica;
  mg.dirty = true;
  return GLS_OK;
}

int gls_mg_attach_replica(gls_ctx *c, const gls_mg_params *p, gls_ctx *replica, const int64_t *p_off,
                          const int32_t *p_col, const double *p_w, const int64_t *inject) {
  GLS_TRY(check_ctx(c));
  if (!p || !replica || replica == c || replica->dist.on || !p_off || !p_col || !p_w || !inject)
    return set_err(GLS_EINVAL, "mg replica attach: arguments");
  if (p->smoother == 3) return set_err(GLS_EINVAL, "mg replica attach: the cell-Vanka smoother (3) runs on one rank only");
  if (!c->dist.on) return set_err(GLS_EINVAL, "mg replica attach: the fine context is not distributed");
  if (replica->dim != c->dim || replica->k != c->k || replica->kp != c->kp)
    return set_err(GLS_EINVAL, "mg replica attach: replica order / dimension differs");
  if (p->smoother < 0 || p->smoother > 1) return set_err(GLS_EINVAL, "mg replica attach: smoother 0 or 1");
  GLS_TRY(gls_mg_detach(c));
  auto &mg = c->mg;
  const int64_t n = c->n_dofs, ng = replica->n_dofs;
  if (ng >= INT32_MAX) return set_err(GLS_EINVAL, "mg replica attach: replica too large");
  const int64_t dv = (int64_t)c->dim * c->n_vnodes;
  auto owned = [&](int64_t i) { return i < dv ? i < (int64_t)c->dim * c->dist.n_owned : i - dv < c->dist.n_owned_p; };
  // P on the local rows; R = the owned rows' P^T (rows = replica DoFs, local fine columns in ascending order)
  const int64_t nnz = p_off[n];
  std::vector<int64_t> roff((size_t)ng + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (p_off[i + 1] < p_off[i]) return set_err(GLS_EINVAL, "mg replica attach: P offsets");
    for (int64_t e = p_off[i]; e < p_off[i + 1]; ++e) {
      if (p_col[e] < 0 || p_col[e] >= ng) return set_err(GLS_EINVAL, "mg replica attach: P column %d", p_col[e]);
      if (owned(i)) ++roff[(size_t)p_col[e] + 1];
    }
  }
  for (int64_t r = 0; r < ng; ++r) roff[(size_t)r + 1] += roff[(size_t)r];
  std::vector<int32_t> rcol((size_t)roff[(size_t)ng]);
  std::vector<double> rw(rcol.size());
  std::vector<int64_t> fill(roff.begin(), roff.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    if (owned(i))
      for (int64_t e = p_off[i]; e < p_off[i + 1]; ++e) {
        const int64_t at = fill[(size_t)p_col[e]]++;
        rcol[(size_t)at] = (int32_t)i;
        rw[(size_t)at] = p_w[e];
      }
  std::vector<int32_t> ic, iff;
  for (int64_t r = 0; r < ng; ++r)
    if (inject[r] >= 0) {
      if (inject[r] >= n || !owned(inject[r])) return set_err(GLS_EINVAL, "mg replica attach: inject[%lld] not owned", (long long)r);
      ic.push_back((int32_t)r);
      iff.push_back((int32_t)inject[r]);
    }
  GLS_TRY(mg.r2p_off.upload(p_off, (size_t)n + 1));
  GLS_TRY(mg.r2p_col.upload(p_col, std::max<size_t>((size_t)nnz, 1)));
  GLS_TRY(mg.r2p_w.upload(p_w, std::max<size_t>((size_t)nnz, 1)));
  GLS_TRY(mg.r2r_off.upload(roff.data(), roff.size()));
  if (rcol.empty()) {
    rcol.push_back(0);
    rw.push_back(0.0);
  }
  GLS_TRY(mg.r2r_col.upload(rcol.data(), rcol.size()));
  GLS_TRY(mg.r2r_w.upload(rw.data(), rw.size()));
  auto lanes = [](double mean) { return mean > 24 ? 16 : mean > 6 ? 4 : 1; };
  mg.r2p_lane = lanes(n ? (double)nnz / (double)n : 0.0);
  mg.r2r_lane = lanes(ng ? (double)(roff[(size_t)ng]) / (double)ng : 0.0);
  if (ic.empty()) {
    ic.push_back(0);
    iff.push_back(0);
  }
  GLS_TRY(mg.r2inj_c.upload(ic.data(), ic.size()));
  GLS_TRY(mg.r2inj_f.upload(iff.data(), iff.size()));
  if (ic.size() == 1 && inject[ic[0]] < 0) mg.r2inj_c.n = mg.r2inj_f.n = 0;  // no owned source on this rank
  GLS_TRY(mg.rep_b.alloc((size_t)ng));
  GLS_TRY(mg.rep_x.alloc((size_t)ng));
  GLS_TRY(mg.rep_tmp.alloc(std::max<size_t>(ic.size(), 1)));
  for (auto &u : mg.rep_u) GLS_TRY(u.alloc((size_t)ng));
  // smoothing on the distributed fine level: damped Jacobi or ILU(0) (per-rank blocks, Ifpack overlap 0)
  mg.lev.assign(1, c);
  mg.pre = p->pre_smooth > 0 ? p->pre_smooth : (p->pre_smooth < 0 ? 0 : 2);
  mg.post = p->post_smooth >= 0 ? p->post_smooth : 2;
  mg.lpre.assign(1, mg.pre);
  mg.lpost.assign(1, mg.post);
  mg.omega = p->omega > 0 ? p->omega : 0.6;
  mg.comega = mg.omega;
  mg.ilu_smooth = p->smoother == 1;
  for (int b = 0; b < MB_N; ++b) {
    mg.bufs.emplace_back(new DevBuf<double>());
    if (b == MB_Y || (b == MB_BOX && mg.ilu_smooth)) GLS_TRY(mg.bufs.back()->alloc((size_t)n));
  }
  if (mg.ilu_smooth) {
    GLS_TRY(gls_ilu_set_options(c, GLS_ILU_ORDER_MULTICOLOR, 0));
    GLS_TRY(gls_ilu_attach(c, 0, 1e-12, 1.0));
    mg.ilu_levels.push_back(c);
  }
  // a replica without a hierarchy of its own is the coarsest level: exact LU when asked (coarse_direct > 0)
  if (p->coarse_direct > 0 && !replica->mg.on) {
    if (ng > 8192) return set_err(GLS_EINVAL, "mg replica attach: direct coarse solve needs <= 8192 DoFs");
    mg.direct = true;
    GLS_TRY(mg.coarse.init(ng));
    GLS_TRY(mg_probe_setup(c, replica));
  }
  if (replica->stream != c->stream) GLS_TRY(gls_set_stream(replica, c->stream));
  mg.rep2 = replica;
  mg.rep_csr = true;
  mg.on = true;
  mg.dirty = true;
  return GLS_OK;
}

int gls_mg_coarse_info(gls_ctx *c, int64_t *n, int *storage, int64_t *bl, int64_t *bu, int64_t *nb, int64_t *bytes) {
  GLS_TRY(check_ctx(c));
  const auto &cs = c->mg.coarse;
  const bool on = c->mg.on && c->mg.direct, band = on && cs.band_store;
  if (n) *n = on ? cs.n : 0;
  if (storage) *storage = band ? 1 : 0;
  if (bl) *bl = band ? cs.blu.L.bl : -1;
  if (bu) *bu = band ? cs.blu.L.bu : -1;
  if (nb) *nb = band ? cs.blu.L.nb : -1;
  if (bytes) *bytes = !on ? 0 : band ? (int64_t)cs.blu.bytes() : (int64_t)(cs.probe.n * sizeof(double) + cs.probe32.n * sizeof(float));
  return GLS_OK;
}

int gls_mg_detach(gls_ctx *c) {
  GLS_TRY(check_ctx(c));
  // a coarse factorization in flight ends first: on the band route its check reads the probing ILU's CSR, which
  // belongs to the coarsest level's context and is released just below
  c->mg.coarse.side.reset();
  for (auto *g : c->mg.lev) g->smooth_f32 = g->smooth_oseen = false;
  // the ILU(0) smoothers the attach put on the levels (level 0 is this context) go with the multigrid, so
  // the preconditioner falls back to Jacobi (gls_native.h) and not to a leftover smoother ILU
  for (auto *g : c->mg.ilu_levels) GLS_TRY(gls_ilu_detach(g));
  for (auto *g : c->mg.lev)  // and the cell-Vanka maps, matrices and inverses of the levels it smoothed
    if (g->vanka.smooth) {
      HIP_TRY(hipStreamSynchronize(g->stream));
      g->vanka = gls_ctx::Vanka();
    }
  c->mg = gls_ctx::MG();  // (CoarseSolve's assignment ends a coarse factorization in flight first)
  return GLS_OK;
}

}  // extern "C"
