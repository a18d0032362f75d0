// gls_ilu.cpp -- the device side of the assembled ILU(k) preconditioner: attach (download, the host-only plan of
// gls_ilu_plan.cpp, across ranks the collective column-tag exchange, uploads, rocSPARSE analysis), probing,
// factorization and the triangular solves. The multigrid's ILU smoother (gls_api.cpp, gls_mg.cpp) calls ensure_ilu / apply_ilu.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gls_ctx.hpp"
#include "gls_ilu_plan.hpp"

using namespace gls_impl;

static_assert(gls::kPlanMaxGroupRows == gls::kMaxGroupRows && gls::kPlanGroupDesc == gls::kGroupDesc,
              "gls_ilu_plan.hpp builds the node-group descriptors the multicolor solve kernels read");

namespace gls_impl {

// assembled ILU(0): probe the operator into the CSR values (one J.v per color and DoF slot), perturb
// the diagonal, factor in place; once per Jacobian state (invalidated with the diagonal)
// the per-cell path on one rank: all probes in batches of B vectors, each step one launch over the batch
// (unit vectors, hanging-line values, the per-cell J.v with zero cell batches skipped, the ordered
// element-vector sums, condensation, constrained rows, extraction) -- the same operations per probe as
// gls_jacobian_apply, without one launch sequence per probe
static int ilu_probe_batched(gls_ctx *c) {
  auto &I = c->ilu;
  const int64_t n = c->n_dofs;
  hipStream_t s = c->stream;
  if (!c->u) return set_err(GLS_EINVAL, "gls_set_state was not called");
  GLS_TRY(ensure_element_maps(c));
  if (c->con_dofs.n) GLS_TRY(ensure_diag(c));
  const int dim = c->dim, nv = gls::ipow(c->k + 1, dim), np = gls::ipow(c->kp + 1, dim);
  const int64_t el = (int64_t)nv * dim + np, evs = (int64_t)c->n_cells * el;
  const char *bs = std::getenv("GLS_ILU_PROBE_BATCH");
  const int64_t budget = (int64_t)1 << 31;  // bytes of V, C V, Y and the element vectors per batch
  int B = bs ? std::atoi(bs) : (int)std::min<int64_t>(I.n_probes, std::max<int64_t>(1, budget / (8 * (3 * n + evs))));
  B = std::max(1, std::min(B, I.n_probes));
  if (I.bV.n < (size_t)B * n) {
    GLS_TRY(I.bV.alloc((size_t)B * n));
    GLS_TRY(I.bY.alloc((size_t)B * n));
  }
  if (c->hang.on && I.bC.n < (size_t)B * n) GLS_TRY(I.bC.alloc((size_t)B * n));
  if (c->bev.n < (size_t)B * evs) GLS_TRY(c->bev.alloc((size_t)B * evs));
  const int cb = gls::cell_kernel_cells_per_block(dim, c->k, c->nq1d, true), nblk = (c->n_cells + cb - 1) / cb;
  if (c->bact.n < (size_t)B * nblk) GLS_TRY(c->bact.alloc((size_t)B * nblk));
  if (I.fill > 0) HIP_TRY(gls::vec_fill(I.val.p, I.nnz, 0.0, s));  // fill-in positions start at 0
  // recorded activity (GLS_ILU_PROBE_LIST=0: every (probe, batch) block tests its vector, every time)
  const char *wl_env = std::getenv("GLS_ILU_PROBE_LIST");
  const bool wl_on = !(wl_env && wl_env[0] == '0');
  const bool use_list = wl_on && !I.woff.empty() && I.wB == B && I.wnblk == nblk;
  const bool record = wl_on && !use_list;
  // listed blocks read u, grad u, tau and R_s from the linearization cache of this state (the diagonal pass writes
  // it for every cell; not on forests, whose cache covers the cells outside the bricks only)
  bool cq_probe = use_list && cell_cache_on(c) && !c->oct.on;
  if (cq_probe) {
    GLS_TRY(ensure_diag(c));
    cq_probe = c->cq_valid && c->cq.n == cell_cache_size(c);
  }
  std::vector<int32_t> hlist;
  std::vector<int64_t> hoff;
  std::vector<uint8_t> hact;
  if (record) {
    GLS_TRY(I.wact.alloc((size_t)I.n_probes * nblk));
    hoff.push_back(0);
  }
  for (int p0 = 0; p0 < I.n_probes; p0 += B) {
    const int nb = std::min(B, I.n_probes - p0);
    HIP_TRY(gls::vec_fill(I.bV.p, (int64_t)nb * n, 0.0, s));
    const int64_t d0 = I.pdoff[(size_t)p0], d1 = I.pdoff[(size_t)(p0 + nb)];
    HIP_TRY(gls::probe_set_batched(I.bV.p, n, I.pdofs.p + d0, I.pdpid.p + d0, p0, d1 - d0, s));
    const double *Cv = I.bV.p;
    if (c->hang.on) {  // C v (hanging entries interpolated from their masters) in a copy: the constrained
      // rows below take the probe vector itself, as gls_jacobian_apply does
      HIP_TRY(gls::vec_copy(I.bC.p, I.bV.p, (int64_t)nb * n, s));
      HIP_TRY(gls::vec_csr_gather_set_b(I.bC.p, c->hang.dof.p, c->hang.ooff.p, c->hang.omaster.p, c->hang.ow.p,
                                        (int64_t)c->hang.dof.n, nb, n, s));
      Cv = I.bC.p;
    }
    gls::OpParams P = make_params(c, true);
    P.v = Cv;
    P.y = I.bY.p;
    P.hmask = c->hang.on ? c->hang.hmask.p : nullptr;
    P.ev = c->bev.p;
    // (the first, recording run re-derives the linearization in every (probe, cell batch) block: with all blocks
    // launched, reading the cache moved more bytes than the state gathers -- configs[4]'s ILU setup ran 1.4 ms per
    // Newton step slower; the listed runs read it, profiles/r05_ab_probe_cache.txt)
    P.bv_stride = n;
    P.bev_stride = evs;
    P.n_probe = nb;
    const int chunk = p0 / B;
    P.bact = use_list ? I.wact.p + (size_t)p0 * nblk : c->bact.p;
    if (use_list) {
      P.work = I.wlist.p + 2 * I.woff[(size_t)chunk];
      P.n_work = (int)(I.woff[(size_t)chunk + 1] - I.woff[(size_t)chunk]);
      if (cq_probe) {
        P.cq = c->cq.p;
        P.cq_mode = 2;
      }
    }
    if (!use_list || P.n_work > 0) {
      TimedLaunch t(c, (int)gls::MODE_JV);
      HIP_TRY(gls::launch_cell_kernel(c->dim, c->k, c->kp, c->nq1d, gls::MODE_JV, P, c->tables, s));
    }
    if (record) {  // this chunk's flags: kept on the device for the gathers, listed on the host
      HIP_TRY(hipMemcpyAsync(I.wact.p + (size_t)p0 * nblk, c->bact.p, (size_t)nb * nblk, hipMemcpyDeviceToDevice, s));
      hact.resize((size_t)nb * nblk);
      HIP_TRY(hipMemcpyAsync(hact.data(), c->bact.p, hact.size(), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (int v = 0; v < nb; ++v)
        for (int64_t b = 0; b < nblk; ++b)
          if (hact[(size_t)v * nblk + b]) {
            hlist.push_back(v);
            hlist.push_back((int32_t)b);
          }
      hoff.push_back((int64_t)hlist.size() / 2);
    }
    HIP_TRY(gls::gather_element_vectors_b(I.bY.p, c->bev.p, c->ev_voff.p, c->ev_vslot.p, c->n_vnodes, c->ev_poff.p,
                                          c->ev_pslot.p, c->n_pnodes, c->dim, nb, n, evs, P.bact, el, cb, nblk, s));
    if (c->hang.on)
      HIP_TRY(gls::vec_csr_condense_b(I.bY.p, c->hang.tm.p, c->hang.toff.p, c->hang.tdof.p, c->hang.tw.p,
                                      (int64_t)c->hang.tm.n, nb, n, s));
    HIP_TRY(gls::vec_gather_scale_set_b(I.bY.p, c->diag.p, I.bV.p, c->con_dofs.p, (int64_t)c->con_dofs.n, nb, n, s));
    const int64_t e0 = I.peoff[(size_t)p0], e1 = I.peoff[(size_t)(p0 + nb)];
    HIP_TRY(gls::probe_extract_batched(I.val.p, I.pent.p + e0, I.prow.p + e0, I.pepid.p + e0, p0, e1 - e0, I.bY.p, n, s));
  }
  if (I.ghost_diag.n) HIP_TRY(gls::vec_set_const_indexed64(I.val.p, I.ghost_diag.p, (int64_t)I.ghost_diag.n, 1.0, s));
  if (record) {
    GLS_TRY(I.wlist.upload(hlist.data(), hlist.size()));
    I.woff.swap(hoff);
    I.wB = B;
    I.wnblk = nblk;
  }
  return GLS_OK;
}

int ilu_probe(gls_ctx *c) {  // I.val <- the operator's CSR values (gls_jacobian_apply)
  auto &I = c->ilu;
  const int64_t n = c->n_dofs;
  hipStream_t s = c->stream;
  if (!c->dist.on && !c->use_brick && !std::getenv("GLS_ILU_PROBE_LOOP")) return ilu_probe_batched(c);
  if (I.fill > 0 || c->dist.on) HIP_TRY(gls::vec_fill(I.val.p, I.nnz, 0.0, s));  // fill-in positions start at 0
  // across ranks the constrained rows' diagonal is the exchanged one: computed before the local probes
  if (c->dist.on && (c->con_dofs.n || I.complete)) GLS_TRY(ensure_diag(c));
  c->probe_local = c->dist.on;  // the probe's J.v: the rank's cells only, no ghost exchange
  struct ProbeLocalGuard {      // every exit path (errors included) restores the exchanging operator
    gls_ctx *c;
    ~ProbeLocalGuard() { c->probe_local = false; }
  } guard{c};
  auto &D = c->dist;
  const int rounds = I.complete ? I.n_rounds : I.n_probes;
  for (int p = 0; p < rounds; ++p) {
    if (p < I.n_probes) {
      HIP_TRY(gls::vec_fill(I.vbuf.p, n, 0.0, s));
      HIP_TRY(gls::vec_set_const_indexed(I.vbuf.p, I.pdofs.p + I.pdoff[(size_t)p],
                                         I.pdoff[(size_t)p + 1] - I.pdoff[(size_t)p], 1.0, s));
      GLS_TRY(gls_jacobian_apply(c, I.vbuf.p, I.ybuf.p));
      HIP_TRY(gls::csr_probe_extract(I.val.p, I.pent.p + I.peoff[(size_t)p], I.prow.p + I.peoff[(size_t)p],
                                     I.peoff[(size_t)p + 1] - I.peoff[(size_t)p], I.ybuf.p, s, c->dist.on));
    }
    if (!I.complete) continue;
    // ghost rows of this probe (the local cells' part of a neighbour's owned rows) to their owners
    if (p < I.n_probes) HIP_TRY(gls::vec_pack_dofs(I.ybuf.p, D.recv_nodes.p, D.n_recv, D.recv_buf, s));
    else if (D.n_recv) HIP_TRY(gls::vec_fill(D.recv_buf, D.n_recv, 0.0, s));
    if (D.xchg(D.user, 1) != 0) return set_err(GLS_ECOMM, "ILU probe exchange failed");
    const int64_t a = I.rr[(size_t)p], b = I.rr[(size_t)p + 1];
    if (b > a) HIP_TRY(gls::vec_add_pos_ordered(I.val.p, I.ru.p + a, I.ruoff.p + a, I.rslot.p, b - a, D.send_buf, s));
  }
  c->probe_local = false;
  if (I.ghost_diag.n) HIP_TRY(gls::vec_set_const_indexed64(I.val.p, I.ghost_diag.p, (int64_t)I.ghost_diag.n, 1.0, s));
  return GLS_OK;
}
int ensure_ilu(gls_ctx *c) {
  auto &I = c->ilu;
  if (!I.on || I.valid) return GLS_OK;
  const int64_t n = c->n_dofs;
  hipStream_t s = c->stream;
  const bool verbose = std::getenv("GLS_ILU_VERBOSE") != nullptr;
  auto now = [&]() {
    if (verbose) (void)hipStreamSynchronize(s);
    return std::chrono::steady_clock::now();
  };
  const auto t0 = now();
  GLS_TRY(ilu_probe(c));
  HIP_TRY(gls::csr_diag_perturb(I.val.p, I.didx.p, n, I.athresh, I.rthresh, s));
  const auto t1 = now();
  const rocsparse_int m = (rocsparse_int)n, nnz = (rocsparse_int)I.nnz;
  if (I.h) RS_TRY(rocsparse_set_stream(I.h, s));  // (no handle past 2^31 entries: multicolor kernels only)
  if (I.mc_factor)
    HIP_TRY(gls::ilu_mc_factor(I.mc_grow.p, I.mc_cg.data(), (int)I.mc_cg.size() - 1, I.rowp.p, I.col.p, I.val.p,
                               I.mc_lsp.p, I.didx.p, I.boost_tol, I.boost_val, I.mc_moff.p,
                               I.mc_map.n ? I.mc_map.p : nullptr, I.mc_compact, I.rdiag.p, s));
  else
    RS_TRY(rocsparse_dcsrilu0(I.h, m, nnz, I.dA, I.val.p, I.rowp32.p, I.col.p, I.info, rocsparse_solve_policy_auto, I.work.p));
  I.valid = true;
  if (verbose) {
    const auto t2 = now();
    rocsparse_int zp = -1;
    const rocsparse_status st = I.h ? rocsparse_csrilu0_zero_pivot(I.h, I.info, &zp) : rocsparse_status_success;
    GLS_TRY(apply_ilu(c, I.ybuf.p, I.ybuf.p == nullptr ? nullptr : c->tmp1.p ? c->tmp1.p : I.ybuf.p));
    const auto t3 = now();
    std::printf("ilu: %d probes %.2f ms, csrilu0 %.2f ms (zero pivot status %d at %d), one apply %.3f ms\n", I.n_probes,
                std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count(), (int)st, (int)zp,
                std::chrono::duration<double, std::milli>(t3 - t2).count());
  }
  return GLS_OK;
}
int apply_ilu(gls_ctx *c, const double *v, double *z) {
  auto &I = c->ilu;
  const rocsparse_int m = (rocsparse_int)c->n_dofs, nnz = (rocsparse_int)I.nnz;
  const double one = 1.0;
  if (I.h) RS_TRY(rocsparse_set_stream(I.h, c->stream));
  // z = P^T U^-1 L^-1 P v (P: the Cuthill-McKee renumbering the factors live in)
  HIP_TRY(gls::vec_permute(I.vbuf.p, v, I.perm.p, c->n_dofs, 0, c->stream));
  if (I.mc_solve) {  // multicolor order: color-by-color solves (gls_ilu_kernels.hip)
    HIP_TRY(gls::ilu_mc_solve(I.mc_desc.p, I.mc_cg.data(), (int)I.mc_cg.size() - 1, I.col.p, I.val.p, I.vbuf.p,
                              I.tbuf.p, I.vbuf.p, I.mc_wl.data(), I.mc_wu.data(), c->stream));
    HIP_TRY(gls::vec_permute(z, I.vbuf.p, I.perm.p, c->n_dofs, 1, c->stream));
    return GLS_OK;
  }
  RS_TRY(rocsparse_dcsrsv_solve(I.h, rocsparse_operation_none, m, nnz, &one, I.dL, I.val.p, I.rowp32.p, I.col.p, I.info,
                                I.vbuf.p, I.tbuf.p, rocsparse_solve_policy_auto, I.work.p));
  RS_TRY(rocsparse_dcsrsv_solve(I.h, rocsparse_operation_none, m, nnz, &one, I.dU, I.val.p, I.rowp32.p, I.col.p, I.info,
                                I.tbuf.p, I.vbuf.p, rocsparse_solve_policy_auto, I.work.p));
  HIP_TRY(gls::vec_permute(z, I.vbuf.p, I.perm.p, c->n_dofs, 1, c->stream));
  return GLS_OK;
}

}  // namespace gls_impl

// ---------------------------------------------------------------------------------------------
// gls_ilu_attach: the reference's ILU-preconditioned GMRES (linear solver method gmres with 'ilu
// preconditioner fill / absolute tolerance / relative tolerance', setup_ILU gls_navier_stokes.cc:
// 1161-1176: Ifpack ILU(k) with athresh / rthresh, no overlap) on the assembled Jacobian. The matrix
// is never formed by a CPU: it is probed from the device operator with distance-2-colored unit
// vectors (no two DoFs of a probe share a row). Its graph is the reference's system-matrix sparsity
// (make_sparsity_pattern with nonzero_constraints, keep_constrained_dofs = false,
// gls_navier_stokes.cc:208-211): a constrained row / column holds its diagonal only, lines
// (hanging nodes, slip on curved walls) couple their masters. The DoFs are renumbered like
// DoFRenumbering::Cuthill_McKee (gls_navier_stokes.cc:70), the level-of-fill pattern of ILU(fill)
// is inserted with explicit zeros, and rocSPARSE csrilu0 on that pattern computes ILU(fill).
// ---------------------------------------------------------------------------------------------
namespace {

// what the plan reads, from the context: the mesh and the constrained DoFs downloaded, the lines' host copy
int ilu_plan_input(gls_ctx *c, int fill, gls::IluPlanInput &in) {
  in.dim = c->dim, in.k = c->k, in.kp = c->kp;
  in.n_vnodes = c->n_vnodes, in.n_pnodes = c->n_pnodes, in.n_cells = c->n_cells;
  in.cell_vnodes.resize((size_t)c->n_cells * gls::ipow(c->k + 1, c->dim));
  HIP_TRY(hipMemcpy(in.cell_vnodes.data(), c->cell_vnodes.p, in.cell_vnodes.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (c->cell_pnodes.p) {
    in.cell_pnodes.resize((size_t)c->n_cells * gls::ipow(c->kp + 1, c->dim));
    HIP_TRY(hipMemcpy(in.cell_pnodes.data(), c->cell_pnodes.p, in.cell_pnodes.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  in.con_dofs.resize(c->con_dofs.n);
  if (!in.con_dofs.empty())
    HIP_TRY(hipMemcpy(in.con_dofs.data(), c->con_dofs.p, in.con_dofs.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (c->hang.on) {
    in.h_dof = c->hang.h_dof;
    in.h_off = c->hang.h_off;
    in.h_master = c->hang.h_master;
  }
  if (c->dist.on) {
    in.n_owned = c->dist.n_owned;
    in.n_owned_p = c->dist.n_owned_p;
  }
  in.fill = fill;
  in.ordering = c->ilu.ordering;
  in.block_dofs = c->ilu.block_dofs;
  return GLS_OK;
}

// Across ranks, complete owned rows: every rank probes its cells' operator on all its DoFs (owned and ghost); the
// ghost rows of each probe go to their owners through the export exchange, tagged once (here) with the column as
// its position in the owner's send list. Probe rounds run to the largest probe count of any rank (collective).
int exchange_column_tags(gls_ctx *c, const gls::IluPlan &P, std::vector<gls::IluRemoteEntry> &remote, int &n_rounds) {
  const int64_t n = c->n_dofs;
  const auto &cons = P.cons;
  const auto &fcons = P.fcons;
  const auto &faoff = P.fa.off;
  const auto &facol = P.fa.col;
  const int nprobe_local = P.n_probes;
  // the column tags: per round, each ghost row's probed column as its position in the owner's list
  auto &D = c->dist;
  const int nn = (int)D.h_soff.size() - 1;
  const int64_t ns = D.n_send, nr = D.n_recv;
  std::vector<int32_t> gnb((size_t)n, -1), gk((size_t)n, -1);
  for (int t = 0; t < nn; ++t)
    for (int64_t q = D.h_roff[(size_t)t]; q < D.h_roff[(size_t)t + 1]; ++q) {
      gnb[(size_t)D.h_recv[(size_t)q]] = t;
      gk[(size_t)D.h_recv[(size_t)q]] = (int32_t)(q - D.h_roff[(size_t)t]);
    }
  std::vector<double> hpos((size_t)std::max<int64_t>(nr, 1)), hin((size_t)std::max<int64_t>(ns, 1));
  for (int p = 0;; ++p) {
    double flag = p < nprobe_local ? 1.0 : 0.0;
    HIP_TRY(hipMemcpy(D.red_buf, &flag, sizeof(double), hipMemcpyHostToDevice));
    if (D.allreduce(D.user, D.red_buf, 1) != 0) return set_err(GLS_ECOMM, "gls_ilu_attach: allreduce failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&flag, D.red_buf, sizeof(double), hipMemcpyDeviceToHost));
    if (flag == 0.0) break;
    ++n_rounds;
    for (int64_t q = 0; q < nr; ++q) {
      const int64_t i = D.h_recv[(size_t)q];
      double pos = -1.0;
      if (p < nprobe_local && !fcons[(size_t)i])
        for (int64_t t = faoff[(size_t)i]; t < faoff[(size_t)i + 1]; ++t) {
          const int64_t j = facol[(size_t)t];
          if (P.probe_of(j) != p) continue;
          if (gnb[(size_t)j] == gnb[(size_t)i]) pos = (double)gk[(size_t)j];
          break;
        }
      hpos[(size_t)q] = pos;
    }
    if (nr) HIP_TRY(hipMemcpy(D.recv_buf, hpos.data(), sizeof(double) * (size_t)nr, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    if (D.xchg(D.user, 1) != 0) return set_err(GLS_ECOMM, "gls_ilu_attach: exchange failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ns) HIP_TRY(hipMemcpy(hin.data(), D.send_buf, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost));
    for (int t = 0; t < nn; ++t)
      for (int64_t q = D.h_soff[(size_t)t]; q < D.h_soff[(size_t)t + 1]; ++q) {
        const int64_t pos = (int64_t)hin[(size_t)q];
        if (pos < 0) continue;
        if (pos >= D.h_soff[(size_t)t + 1] - D.h_soff[(size_t)t]) return set_err(GLS_ECOMM, "gls_ilu_attach: bad column tag");
        const int64_t i = D.h_send[(size_t)q], j = D.h_send[(size_t)(D.h_soff[(size_t)t] + pos)];
        if (cons[(size_t)i] || cons[(size_t)j]) continue;
        remote.push_back({p, (int32_t)q, i, j});
      }
  }
  return GLS_OK;
}

}  // namespace

extern "C" int gls_ilu_attach(gls_ctx *c, int fill, double athresh, double rthresh) {
  GLS_TRY(check_ctx(c));
  auto &I = c->ilu;
  I.probe_only = false;  // a caller's attach: a preconditioner (mg_probe_setup marks its own afterwards)
  if (c->dist.on && !c->dist.dofs) return set_err(GLS_EINVAL, "gls_ilu_attach: brick-partitioned contexts use the multigrid");
  if (c->mg.on) return set_err(GLS_EINVAL, "gls_ilu_attach: a multigrid preconditioner is attached");
  if (fill < 0 || fill > GLS_ILU_MAX_FILL)
    return set_err(GLS_EINVAL, "gls_ilu_attach: ilu preconditioner fill %d not supported (0..%d)", fill, GLS_ILU_MAX_FILL);
  const int64_t n = c->n_dofs;
  if (n >= INT32_MAX) return set_err(GLS_EINVAL, "gls_ilu_attach: too many DoFs for 32-bit CSR");
  // the plan (host only): patterns and probe colours; across ranks the collective tag exchange; everything else
  gls::IluPlanInput in;
  GLS_TRY(ilu_plan_input(c, fill, in));
  gls::IluPlan P;
  std::string err;
  if (gls::ilu_plan_patterns(in, P, err) != 0) return set_err(GLS_EINVAL, "%s", err.c_str());
  std::vector<gls::IluRemoteEntry> remote;
  int n_rounds = 0;
  if (P.complete) GLS_TRY(exchange_column_tags(c, P, remote, n_rounds));
  if (gls::ilu_plan_finish(in, remote, n_rounds, P, err) != 0) return set_err(GLS_EINVAL, "%s", err.c_str());
  // multicolor solves where the plan found them valid; which factorization runs, and whether its position map
  // (uint16 per entry) fits a quarter of free memory, is decided here
  I.mc_solve = P.mc_solve;
  I.mc_factor = false;
  I.mc_compact = false;
  if (in.ordering == GLS_ILU_ORDER_MULTICOLOR) I.n_order_colors = P.n_order_colors;
  bool factor_map = false;
  if (P.mc_solve) {
    GLS_TRY(I.mc_grow.upload(P.grow.data(), P.grow.size()));
    GLS_TRY(I.mc_lsp.upload(P.lsp.data(), P.lsp.size()));
    GLS_TRY(I.mc_usp.upload(P.usp.data(), P.usp.size()));
    GLS_TRY(I.mc_desc.upload(P.desc.data(), P.desc.size()));
    I.mc_cg = P.cg;
    I.mc_wl = P.mc_wl;
    I.mc_wu = P.mc_wu;
    I.mc_factor = P.maxrow <= gls::kIluMaxRow && P.rowp.back() < (int64_t(1) << 35) && !std::getenv("GLS_ILU_ROCSPARSE_FACTOR");
    I.mc_compact = P.maxrow <= gls::kIluCompactRow;
    if (I.mc_factor) {
      GLS_TRY(I.rdiag.alloc((size_t)n));
      size_t fr = 0, tot = 0;
      const char *me = std::getenv("GLS_ILU_FACTOR_MAP");
      factor_map = !((me && std::atoi(me) == 0) || hipMemGetInfo(&fr, &tot) != hipSuccess ||
                     (double)P.moff[(size_t)n] * 2.0 > 0.25 * (double)fr);
    }
  }
  I.release();
  GLS_TRY(I.rowp.upload(P.rowp.data(), P.rowp.size()));
  GLS_TRY(I.col.upload(P.col.data(), P.col.size()));
  GLS_TRY(I.didx.upload(P.didx.data(), P.didx.size()));
  GLS_TRY(I.perm.upload(P.perm.data(), P.perm.size()));
  I.mc_map.release();
  I.mc_moff.release();
  if (factor_map) {
    GLS_TRY(I.mc_moff.upload(P.moff.data(), P.moff.size()));
    GLS_TRY(I.mc_map.alloc((size_t)P.moff.back() + 256));  // + the clamped index of empty stages
    HIP_TRY(gls::ilu_mc_factor_map(n, I.rowp.p, I.col.p, I.mc_lsp.p, I.didx.p, I.mc_moff.p, I.mc_map.p, c->stream));
  }
  GLS_TRY(I.ghost_diag.upload(P.ghost_diag.data(), P.ghost_diag.size()));
  GLS_TRY(I.ru.upload(P.ru.data(), P.ru.size()));
  GLS_TRY(I.ruoff.upload(P.ruoff.data(), P.ruoff.size()));
  GLS_TRY(I.rslot.upload(P.rslot.data(), P.rslot.size()));
  I.rr = P.rr;
  I.complete = P.complete;
  I.n_rounds = n_rounds;
  GLS_TRY(I.pdofs.upload(P.pdofs.data(), P.pdofs.size()));
  GLS_TRY(I.pent.upload(P.pent.data(), P.pent.size()));
  GLS_TRY(I.prow.upload(P.prow.data(), P.prow.size()));
  GLS_TRY(I.pdpid.upload(P.pdpid.data(), P.pdpid.size()));
  GLS_TRY(I.pepid.upload(P.pepid.data(), P.pepid.size()));
  GLS_TRY(I.val.alloc(P.col.size() + 256));  // + the factorization's whole-quad loads past a row's end
  HIP_TRY(hipMemset(I.val.p, 0, P.col.size() * sizeof(double)));
  GLS_TRY(I.vbuf.alloc((size_t)n));
  GLS_TRY(I.ybuf.alloc((size_t)n));
  GLS_TRY(I.tbuf.alloc((size_t)n));
  I.pdoff = P.pdoff;
  I.woff.clear();  // new probes: their activity is recorded again
  I.peoff = P.peoff;
  I.n_probes = P.n_probes;
  I.nnz = (int64_t)P.col.size();
  I.nnz_a = P.nnz_a;
  I.fill = fill;
  I.n_blocks = P.n_blocks;
  I.athresh = athresh;
  I.rthresh = rthresh;
  // the multicolor kernels factor and solve: no rocSPARSE state (its csrilu0 / csrsv analyses were a setup cost of
  // ~0.9 s at 1.7 M DoFs, a radix sort each, for solves that never ran); past 2^31 entries they are the only route
  // (rocSPARSE takes 32-bit CSR)
  if (I.nnz >= INT32_MAX || (I.mc_factor && I.mc_solve)) {
    if (!I.mc_factor || !I.mc_solve)
      return set_err(GLS_EINVAL, "gls_ilu_attach: %lld entries (> 2^31): the multicolor order with fill 0 is needed",
                     (long long)I.nnz);
    I.boost_tol = athresh > 0 ? athresh : 1e-300;  // as below, read by the multicolor factorization
    I.boost_val = athresh > 0 ? athresh : 1e-12;
    I.valid = false;
    I.on = true;
    return GLS_OK;
  }
  {
    std::vector<int32_t> rp32(P.rowp.begin(), P.rowp.end());
    GLS_TRY(I.rowp32.upload(rp32.data(), rp32.size()));
  }
  RS_TRY(rocsparse_create_handle(&I.h));
  RS_TRY(rocsparse_set_stream(I.h, c->stream));
  RS_TRY(rocsparse_create_mat_descr(&I.dA));
  RS_TRY(rocsparse_create_mat_descr(&I.dL));
  RS_TRY(rocsparse_set_mat_fill_mode(I.dL, rocsparse_fill_mode_lower));
  RS_TRY(rocsparse_set_mat_diag_type(I.dL, rocsparse_diag_type_unit));
  RS_TRY(rocsparse_create_mat_descr(&I.dU));
  RS_TRY(rocsparse_set_mat_fill_mode(I.dU, rocsparse_fill_mode_upper));
  RS_TRY(rocsparse_set_mat_diag_type(I.dU, rocsparse_diag_type_non_unit));
  RS_TRY(rocsparse_create_mat_info(&I.info));
  const rocsparse_int m = (rocsparse_int)n, nnz = (rocsparse_int)I.nnz;
  size_t b0 = 0, b1 = 0, b2 = 0;
  RS_TRY(rocsparse_dcsrilu0_buffer_size(I.h, m, nnz, I.dA, I.val.p, I.rowp32.p, I.col.p, I.info, &b0));
  RS_TRY(rocsparse_dcsrsv_buffer_size(I.h, rocsparse_operation_none, m, nnz, I.dL, I.val.p, I.rowp32.p, I.col.p, I.info, &b1));
  RS_TRY(rocsparse_dcsrsv_buffer_size(I.h, rocsparse_operation_none, m, nnz, I.dU, I.val.p, I.rowp32.p, I.col.p, I.info, &b2));
  GLS_TRY(I.work.alloc(std::max(std::max(b0, b1), std::max(b2, (size_t)16))));
  RS_TRY(rocsparse_dcsrilu0_analysis(I.h, m, nnz, I.dA, I.val.p, I.rowp32.p, I.col.p, I.info, rocsparse_analysis_policy_reuse,
                                     rocsparse_solve_policy_auto, I.work.p));
  RS_TRY(rocsparse_dcsrsv_analysis(I.h, rocsparse_operation_none, m, nnz, I.dL, I.val.p, I.rowp32.p, I.col.p, I.info,
                                   rocsparse_analysis_policy_reuse, rocsparse_solve_policy_auto, I.work.p));
  RS_TRY(rocsparse_dcsrsv_analysis(I.h, rocsparse_operation_none, m, nnz, I.dU, I.val.p, I.rowp32.p, I.col.p, I.info,
                                   rocsparse_analysis_policy_reuse, rocsparse_solve_policy_auto, I.work.p));
  // pivots that end below athresh in magnitude are boosted to athresh (enclosed-flow pressure mode)
  // (rocsparse stores the two pointers and reads them at every csrilu0: they must outlive this call;
  // stack locals here gave the first factorization whatever the stack later held)
  I.boost_tol = athresh > 0 ? athresh : 1e-300;
  I.boost_val = athresh > 0 ? athresh : 1e-12;
  RS_TRY(rocsparse_dcsrilu0_numeric_boost(I.h, I.info, 1, &I.boost_tol, &I.boost_val));
  I.on = true;
  I.valid = false;
  if (std::getenv("GLS_ILU_VERBOSE"))
    std::printf("ilu attach: n %lld fill %d blocks %d ordering %s (%d colors%s) nnz(A) %lld nnz(ILU) %lld probe colors "
                "%d probes %d\n", (long long)n, fill, P.n_blocks, I.ordering == GLS_ILU_ORDER_CM ? "cuthill-mckee" : "multicolor",
                I.n_order_colors, I.mc_solve ? ", color solves" : "", (long long)I.nnz_a, (long long)I.nnz,
                P.n_probe_colors, P.n_probes);
  return GLS_OK;
}
extern "C" int gls_ilu_set_options(gls_ctx *c, int ordering, int64_t block_dofs) {
  GLS_TRY(check_ctx(c));
  if (block_dofs < 0) return set_err(GLS_EINVAL, "gls_ilu_set_options: negative block size");
  if (ordering != GLS_ILU_ORDER_CM && ordering != GLS_ILU_ORDER_MULTICOLOR)
    return set_err(GLS_EINVAL, "gls_ilu_set_options: ordering %d", ordering);
  c->ilu.block_dofs = block_dofs;
  c->ilu.ordering = ordering;
  return GLS_OK;
}
extern "C" int gls_ilu_detach(gls_ctx *c) {
  GLS_TRY(check_ctx(c));
  c->ilu.on = false;
  c->ilu.probe_only = false;
  c->ilu.release();
  return GLS_OK;
}
// the probed (unfactored, unperturbed) operator matrix, for tests: host CSR arrays of gls_ilu_info's nnz
extern "C" int gls_ilu_matrix(gls_ctx *c, int32_t *rowp, int32_t *col, double *val) {
  GLS_TRY(check_ctx(c));
  auto &I = c->ilu;
  if (!I.on) return set_err(GLS_EINVAL, "no ILU attached");
  GLS_TRY(ilu_probe(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // renumbered CSR on the device; returned in the context's DoF numbering
  const int64_t n = c->n_dofs;
  if (I.nnz >= INT32_MAX) return set_err(GLS_EINVAL, "gls_ilu_matrix: %lld entries do not fit its 32-bit CSR", (long long)I.nnz);
  std::vector<int64_t> rp((size_t)n + 1);
  std::vector<int32_t> cl((size_t)I.nnz), pm((size_t)n);
  std::vector<double> vl((size_t)I.nnz);
  HIP_TRY(hipMemcpy(rp.data(), I.rowp.p, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cl.data(), I.col.p, sizeof(int32_t) * cl.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(vl.data(), I.val.p, sizeof(double) * vl.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pm.data(), I.perm.p, sizeof(int32_t) * pm.size(), hipMemcpyDeviceToHost));
  std::vector<int32_t> old((size_t)n);
  for (int64_t i = 0; i < n; ++i) old[(size_t)pm[(size_t)i]] = (int32_t)i;
  std::vector<std::vector<std::pair<int32_t, double>>> rows((size_t)n);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e) rows[(size_t)old[(size_t)r]].push_back({old[(size_t)cl[(size_t)e]], vl[(size_t)e]});
  int64_t k = 0;
  if (rowp) rowp[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    std::sort(rows[(size_t)i].begin(), rows[(size_t)i].end());
    for (auto &pr : rows[(size_t)i]) {
      if (col) col[k] = pr.first;
      if (val) val[k] = pr.second;
      ++k;
    }
    if (rowp) rowp[i + 1] = (int32_t)k;
  }
  I.valid = false;  // the values now hold the unfactored matrix
  return GLS_OK;
}
// the factored ILU(fill) (after the diagonal perturbation) in the factorization's numbering, for
// tests: perm[dof] = its row; rowp / col / val of gls_ilu_info's nnz entries (unit-diagonal L below
// the diagonal, U on and above it, as rocSPARSE csrilu0 stores them)
extern "C" int gls_ilu_factors(gls_ctx *c, int32_t *perm, int32_t *rowp, int32_t *col, double *val) {
  GLS_TRY(check_ctx(c));
  auto &I = c->ilu;
  if (!I.on) return set_err(GLS_EINVAL, "no ILU attached");
  GLS_TRY(ensure_diag(c));
  GLS_TRY(ensure_ilu(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (perm) HIP_TRY(hipMemcpy(perm, I.perm.p, sizeof(int32_t) * (size_t)c->n_dofs, hipMemcpyDeviceToHost));
  if (I.nnz >= INT32_MAX) return set_err(GLS_EINVAL, "gls_ilu_factors: %lld entries do not fit its 32-bit CSR", (long long)I.nnz);
  if (rowp) {
    std::vector<int64_t> rp((size_t)c->n_dofs + 1);
    HIP_TRY(hipMemcpy(rp.data(), I.rowp.p, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rp.size(); ++i) rowp[i] = (int32_t)rp[i];
  }
  if (col) HIP_TRY(hipMemcpy(col, I.col.p, sizeof(int32_t) * (size_t)I.nnz, hipMemcpyDeviceToHost));
  if (val) HIP_TRY(hipMemcpy(val, I.val.p, sizeof(double) * (size_t)I.nnz, hipMemcpyDeviceToHost));
  return GLS_OK;
}
extern "C" int gls_ilu_info(const gls_ctx *c, int64_t *nnz, int *n_probes) {
  if (!c) return set_err(GLS_EINVAL, "null context");
  if (nnz) *nnz = c->ilu.nnz;
  if (n_probes) *n_probes = c->ilu.n_probes;
  return c->ilu.on ? GLS_OK : set_err(GLS_EINVAL, "no ILU attached");
}
