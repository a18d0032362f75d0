// gls_ctx.hpp -- internal header of the library's host side (not installed, not part of include/): the context
// struct behind the C-ABI's opaque gls_ctx, the device buffer and error macros every host translation unit uses
// (gls_devbuf.hpp), and the helpers that more than one of them needs (namespace gls_impl; each is defined in the
// file named).
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include <rocblas/rocblas.h>
#include <rocsparse/rocsparse.h>
#include <rccl/rccl.h>

#include "../../include/gls_native.h"
#include "gls_common.hpp"
#include "gls_devbuf.hpp"
#include "gls_error.hpp"
#include "gls_launch.hpp"
#include "gls_mg_coarse.hpp"

#define RS_TRY(x)                                                                        \
  do {                                                                                   \
    const rocsparse_status rs_ = (x);                                                    \
    if (rs_ != rocsparse_status_success) return ::gls_impl::set_err(GLS_EHIP, "%s: rocsparse status %d", #x, (int)rs_); \
  } while (0)

using gls_impl::DevBuf;

struct gls_ctx {
  int dim = 0, k = 0, kp = 0, nq1d = 0, n_cells = 0, n_vnodes = 0, n_pnodes = 0, nq = 0;
  int64_t n_dofs = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  gls::Tables1D tables;
  DevBuf<int32_t> cell_vnodes, cell_pnodes;
  DevBuf<int32_t> face_nbr;  // [n_cells][2 dim] face neighbours (Kelly), built on first use
  DevBuf<double> geo, x0, force_q;
  DevBuf<double> gq;               // mapped cells: per-q geometry [n_cells][nq][kGeo] (nullptr: boxes)
  // gls_flow_diagnostics, allocated at its first call: cell->measure(), the 1D tables, block partials, result
  DevBuf<double> fd_meas, fd_tab, fd_partial, fd_out;
  std::vector<double> host_x0, host_h, host_support;  // host geometry for gls_quadrature_points
  int map_degree = 0;
  DevBuf<uint8_t> vmask;
  DevBuf<int64_t> con_dofs;  // zero_constraints DoF list
  DevBuf<int64_t> dir_dofs;  // nonzero_constraints (Dirichlet) list
  DevBuf<double> dir_vals;
  double viscosity = 1.0;
  int srf = 0;
  double omega[3] = {0, 0, 0};
  // time state
  int scheme = GLS_STEADY;
  double alpha[4] = {0, 0, 0, 0}, alpha_jac = 0., sdt2 = 0.;
  int n_hist = 0;
  // evaluation state (borrowed device pointers)
  const double *u = nullptr, *u1 = nullptr, *u2 = nullptr, *u3 = nullptr;
  DevBuf<double> diag;  // diagonal at the current state (also D_c for constrained rows)
  bool diag_valid = false;
  DevBuf<double> qdata;   // brick J.v linearization at the quadrature points (MODE_LIN output)
  bool qd_valid = false;  // invalidated with the diagonal by every state / parameter change
  // per-cell kernels: linearization cache (u, grad u, tau, R_s per quadrature point) written by the diagonal
  // pass and read by the J.v (OpParams::cq); valid with qd_valid's rules
  DevBuf<double> cq;
  bool cq_valid = false;
  uint64_t cq_epoch = 0;  // counts the diagonal passes that rewrote the cache: what is derived from it (vanka) compares
  DevBuf<float> qdata32;  // FP32 copy of qdata: the multigrid smoother's J.v (mixed precision)
  bool qd32_valid = false;  // stale whenever qdata is recomputed
  bool qd32_partial = false;  // the FP32 copy holds only u and tau (written for the Oseen smoother operator)
  // per-cell path: element vectors and each node's slots in them (deterministic scatter)
  DevBuf<double> ev;
  DevBuf<double> bev;  // batched ILU probing: element vectors of a batch of probe vectors
  DevBuf<uint8_t> bact;  // ... and which (probe, cell batch) blocks computed them
  DevBuf<int64_t> ev_voff, ev_vslot, ev_poff, ev_pslot;
  bool smooth_f32 = false;  // this level's V-cycle J.v runs in FP32 (gls_mg_params.mixed_precision)
  bool smooth_oseen = false;  // ... with the Oseen (Picard) operator (gls_mg_params.smoother_operator = 1)
  bool use_qdata = true;  // GLS_JV_RECOMPUTE=1 -> J.v recomputes the state per call (MODE_JV)
  // solver workspace
  DevBuf<double> work, scal, coef;  // multidot partials, device dot results, GMRES coefficients
  DevBuf<double> scal2;  // GMRES: the projection pass's dots (scal holds the coefficients it reads)
  double *hpin = nullptr;  // pinned host copy of the Gram-Schmidt dots (async D2H, one wait per pass pair)
  size_t hpin_n = 0;
  DevBuf<double> krylov;      // (restart+1) x n_dofs
  DevBuf<double> zbasis;      // restart x n_dofs: M^-1 v_j when the preconditioner is the V-cycle
  DevBuf<double> bicg;        // 7 x n_dofs BiCGStab work vectors (when the GMRES basis is smaller)
  int krylov_m = 0;
  // Newton's ||rhs||^2 for the solve that follows it (device_dot of that very vector; gls_solve_linear takes it for
  // its own device_dot(b, b) when b is this pointer and clears it; gls_set_state and the residual evaluations clear
  // it: the vector is rewritten there)
  const double *bnorm2_of = nullptr;
  double bnorm2_val = 0.;
  DevBuf<double> tmp1, tmp2, tmp3, tmp4, tmp5;
  bool use_brick = false;  // sum-factorized brick kernels (3D Qk-Qk, Morton 2x2x2 bricks)
  // brick-boundary node sums without atomics: each brick stores its partial sums of its NBND
  // surface nodes into a slab; k_slab_sum adds a node's slots in a fixed order (CSR node -> slots)
  bool use_slab = false;
  DevBuf<double> slab;
  DevBuf<double> slab2;  // the fused residual + linearization pass: the residual's brick-surface slab
  DevBuf<int32_t> sum_nodes, sum_off, sum_slots;
  int cube_nb1 = 0;  // > 0: the mesh is the structured hyper_cube with cube_nb1 bricks per direction
                     // (k_slab_sum_cube computes the slab slots from the lattice, the Q2 pencil kernels their
                     // brick nodes' ids, OpParams::cube_gather; GLS_SLAB_CSR=1: off)
  // > 0: the mesh is the open subdivided hyper_rectangle of gls_mesh_hyper_rectangle, box_nb[a] bricks per axis in
  // tile-Morton order with tiles of box_s^3 bricks (gls_box_mesh.hpp; verified cell by cell). Read only where
  // cube_nb1 == 0: k_slab_sum_box computes the slab slots from the lattice. GLS_SLAB_CSR=1: off
  int box_nb[3] = {0, 0, 0};
  int box_s = 0;
  // colored brick launches (opt-in GLS_BRICK_COLORS=1): bricks greedily colored in Morton order so
  // that no two bricks of a color share a node (the 2x2x2 parity classes on a brick lattice: 8
  // colors); surface-node sums carried across colors in acc, no slab and no k_slab_sum. Measured
  // slower at Q2 128^3 (profiles/r02_brick_colors_ab.txt: J.v 3.66 vs 3.00 + 0.55 ms, FP32 3.18 vs
  // 2.44 + 0.45 ms): a color's bricks are not neighbours, so the surface nodes neighbouring bricks
  // share are fetched again from HBM by the later colors instead of hitting L2.
  bool use_colors = false;
  int n_colors = 0;
  int color_off[17] = {0};
  DevBuf<int32_t> color_bricks;
  DevBuf<uint16_t> ncolor;
  DevBuf<double> acc;  // running sums for the fused Jacobi sweep (which stores x, not A x)
  // distributed (rank-local mesh): owned nodes [0, n_owned), ghosts after; exchange via callbacks
  struct Dist {
    bool on = false;
    // dofs: DoF-level exchange of a general mesh (gls_dist_attach_dofs: one double per DoF, owned
    // velocity nodes [0, n_owned) and owned pressure nodes [0, n_owned_p) first); else node-level
    // exchange of a Morton brick mesh (4 doubles per node)
    bool dofs = false;
    int width = 4;  // doubles per exchange entry
    int64_t n_owned = 0, n_owned_p = 0, n_send = 0, n_recv = 0;
    DevBuf<int32_t> add_u, add_off, add_slot;  // export-add (node or DoF exchange) in a fixed order
    DevBuf<int32_t> send_nodes, recv_nodes;
    double *send_buf = nullptr, *recv_buf = nullptr, *red_buf = nullptr;
    gls_exchange_fn xchg = nullptr;
    gls_allreduce_fn allreduce = nullptr;
    void *user = nullptr;
    // in-library RCCL transport (gls_dist_attach_rccl): grouped ncclSend / ncclRecv and ncclAllReduce
    // enqueued on the context stream -- no host callback, no host synchronisation per exchange
    ncclComm_t comm = nullptr;
    std::vector<int> nbrs;
    std::vector<int64_t> soff, roff;
    std::vector<int32_t> h_send, h_recv;  // host copies of the DoF exchange lists (gls_dist_attach_dofs)
    std::vector<int64_t> h_soff, h_roff;
    DevBuf<double> own_send, own_recv, own_red;
    // overlap of the J.v ghost import with the interior bricks (RCCL transport): exchange stream
    hipStream_t xstream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
  } dist;
  // brick split for the overlapped J.v: bricks touching a ghost or exported node first
  // (split[0 .. split_bnd)), then the interior bricks (split[split_bnd .. split_bnd + split_int))
  DevBuf<int32_t> split;
  int split_bnd = 0, split_int = 0;
  // assembled ILU(0) preconditioner (gls_ilu_attach; the reference's setup_ILU,
  // gls_navier_stokes.cc:1161-1176): the Jacobian is assembled into CSR by probing the matrix-free
  // operator with distance-2-colored unit vectors, perturbed on the diagonal like Ifpack (athresh,
  // rthresh) and factored in place by rocSPARSE; M^-1 v = U^-1 L^-1 v (two sparse triangular solves)
  struct ILU {
    bool on = false, valid = false;
    // attached by the multigrid for its coarse matrix's probing pattern only (mg_probe_setup): never factored or
    // applied as a preconditioner / smoother of this context
    bool probe_only = false;
    double athresh = 0., rthresh = 1.;
    double boost_tol = 0., boost_val = 0.;  // rocsparse keeps these POINTERS and reads them in csrilu0
    int n_probes = 0, fill = 0;
    int64_t block_dofs = 0;  // subdomain size of the block-Jacobi ILU (gls_ilu_set_options); 0: one block
    int ordering = GLS_ILU_ORDER_CM, n_blocks = 1, n_order_colors = 0;
    // multicolor order with a pattern whose same-color entries stay inside a node (fill 0): the
    // color-by-color solves of gls_ilu_kernels.hip replace rocSPARSE csrsv
    bool mc_solve = false;
    bool mc_factor = false;  // multicolor order: color-by-color numeric factorization (no rocSPARSE csrilu0)
    bool mc_compact = false;  // ... by the compact-LDS kernel (rows <= kIluCompactRow)
    DevBuf<double> rdiag;     // ... its 1 / U_ii per row
    std::vector<uint8_t> mc_wl, mc_wu;  // per color: wavefronts per node group in the lower / upper solve
    DevBuf<int64_t> mc_desc;   // per node group: the solves' descriptor (gls::kGroupDesc int64)
    DevBuf<int64_t> mc_moff;   // factorization position map: per row, its first entry
    DevBuf<uint16_t> mc_map;   // per (row, pivot, upper entry of the pivot row): position in the row
    std::vector<int32_t> mc_cg;          // per color: first node group (host, n_colors + 1)
    DevBuf<int32_t> mc_grow;             // node group -> first row
    DevBuf<int64_t> mc_lsp, mc_usp;      // per row: L / U split entries
    DevBuf<int64_t> ghost_diag;          // across ranks: diagonal entries of the ghost (identity) rows
    // across ranks, complete owned rows: the neighbours' cell contributions to the owned x owned block
    // arrive per probe round through the export exchange (n_rounds = the largest probe count of any
    // rank); round p adds send_buf slots into CSR entries ru[rr[p] .. rr[p+1]) in a fixed order
    bool complete = false;
    int n_rounds = 0;
    std::vector<int64_t> rr;
    DevBuf<int64_t> ru;
    DevBuf<int32_t> ruoff, rslot;
    std::vector<int64_t> pdoff, peoff;   // per probe: offsets into pdofs and (pent, prow)
    DevBuf<int32_t> pdofs, prow;         // probe unit DoFs; the rows of the CSR entries filled by the probe
    DevBuf<int64_t> pent;                // those entries (positions: 64-bit, the fine levels pass 2^31 entries)
    DevBuf<int32_t> pdpid, pepid;        // probe of each unit DoF / each extracted entry (batched probing)
    DevBuf<double> bV, bC, bY;           // batched probing: probe vectors, C V (hanging lines), results [batch][n_dofs]
    // batched probing's activity: which (probe, cell batch) pairs have a nonzero C e_p on their cells depends on
    // the pattern and the hanging lines only, so the first probing records it (the kernel's flags, wact) and the
    // later ones launch just the active pairs (wlist, per chunk from woff; chunk size wB, batches wnblk)
    DevBuf<uint8_t> wact;
    DevBuf<int32_t> wlist;
    std::vector<int64_t> woff;
    int wB = 0;
    int64_t wnblk = 0;
    // CSR pattern (Cuthill-McKee or multicolor order), diagonal entry per row: 64-bit positions (a 13 M-DoF Q2-Q1
    // level has ~2.9e9 entries); rowp32: the 32-bit row pointers rocSPARSE takes, when the pattern fits them
    DevBuf<int64_t> rowp, didx;
    DevBuf<int32_t> col, rowp32;
    DevBuf<int32_t> perm;                // DoF -> its row in the factored (renumbered) matrix
    DevBuf<double> val, vbuf, ybuf, tbuf;
    DevBuf<char> work;
    rocsparse_handle h = nullptr;
    rocsparse_mat_descr dA = nullptr, dL = nullptr, dU = nullptr;
    rocsparse_mat_info info = nullptr;
    int64_t nnz = 0, nnz_a = 0;  // entries of the ILU(fill) pattern / of the system matrix
    void release() {
      if (info) rocsparse_destroy_mat_info(info);
      if (dA) rocsparse_destroy_mat_descr(dA);
      if (dL) rocsparse_destroy_mat_descr(dL);
      if (dU) rocsparse_destroy_mat_descr(dU);
      if (h) rocsparse_destroy_handle(h);
      info = nullptr;
      dA = dL = dU = nullptr;
      h = nullptr;
    }
    ~ILU() { release(); }
  } ilu;
  // additive cell-Vanka smoother (gls_vanka_host.cpp; gls_mg_params.smoother = 3 and the gls_vanka_* building blocks): the
  // mesh maps built once on the host, and per Jacobian state the element matrices K, the patch matrices A and their
  // FP32 inverses
  struct Vanka {
    bool on = false;      // maps uploaded
    bool smooth = false;  // this level's multigrid smoother (set by the attach, cleared by gls_mg_detach)
    bool valid = false;   // the inverses belong to the cache of epoch `epoch`
    uint64_t epoch = 0;
    int nd = 0;
    DevBuf<int32_t> cell_dofs, nb_cell, flag;
    DevBuf<int64_t> nb_off, ov_off;
    DevBuf<uint8_t> ov_i, ov_j, con;  // con [n_dofs]: 1 on the zero_constraints DoFs
    DevBuf<double> A;     // the patch matrices, kept only once gls_vanka_patch_inverses asked for them (keep_A)
    bool keep_A = false;
    DevBuf<double> r;  // gls_vanka_sweep's residual (the V-cycle passes its own scratch)
    DevBuf<float> Ainv;
    double setup_s = 0.;  // host wall seconds of the last rebuild (GLS_MG_VERBOSE)
  } vanka;
  // hanging-node constraints (gls_set_hanging): lines dof <- sum w * master
  struct Hang {
    bool on = false;
    DevBuf<int64_t> dof, off, master, ooff, omaster;  // all lines; operator lines (Dirichlet masters dropped)
    DevBuf<double> w, ow;
    DevBuf<int64_t> tm, toff, tdof;                     // operator lines transposed: master -> (hanging dof, w)
    DevBuf<double> tw;
    DevBuf<uint8_t> hmask;                             // hanging velocity components per node
    DevBuf<uint8_t> dmask;                             // 1 on the hanging DoFs (C v in one pass)
    DevBuf<double> vbuf;                               // C v for J.v
    std::vector<int64_t> h_dof, h_off, h_master;       // host copy of the lines (ILU sparsity)
  } hang;
  // adapted forests (hanging contexts, 3D Q2-Q2 boxes): the complete sibling groups of leaves run the
  // pencil kernel (cached linearization, element-vector output), the other cells the per-cell kernel
  struct Oct {
    bool on = false;
    int nb = 0;
    DevBuf<int32_t> cell0, list;  // first cell of each brick; 0..nb-1 (the launch's brick list)
    DevBuf<int32_t> rest;         // the cells outside the bricks (the per-cell kernel's list)
    int n_rest = 0;
    bool f32_next = false;        // the next J.v: the bricks in FP32 from qdata32 (the V-cycle's smoother)
  } oct;
  // embedding in the global hyper_cube node lattice (gls_set_lattice): box of local nodes
  struct Lattice {
    bool set = false;
    int n1d = 0, box0[3] = {0, 0, 0}, bdim[3] = {0, 0, 0};
    DevBuf<int32_t> map;  // box node (x fastest) -> local node
  } lat;
  // geometric multigrid preconditioner (levels[0] == this context)
  struct MG {
    bool on = false;
    bool boxed = false;    // distributed levels: transfers go through box gather / scatter
    std::vector<gls_ctx *> lev;
    std::vector<std::array<int, 3>> dims;  // box lattice nodes per direction per level
    int k = 2, pre = 2, post = 2, csweeps = 30;
    std::vector<int> lpre, lpost;  // per-level sweep counts (default pre / post)
    double omega = 0.6, comega = 0.6;
    std::vector<std::unique_ptr<DevBuf<double>>> bufs;  // per level l>=1: u,u1,u2,u3,b,x,y ; level 0: y
    // per level pair (l, l+1) and axis: 1D tap tables [n_out][5] of prolongation / restriction
    struct Taps {
      DevBuf<int32_t> pi[3], ri[3], pc[3], rc[3];
      DevBuf<double> pw[3], rw[3];
      bool two_pass = false;  // the xy tiles of mg_transfer_2pass fit these tables
      // Q2: every axis' taps are the brick-local 5 <-> 3 table the pencil J.v's in-kernel restriction uses
      // (fine nodes 4 c .. 4 c + 4 from coarse nodes 2 c .. 2 c + 2: 1 | 3/8 3/4 -1/8 | 1 | -1/8 3/4 3/8 | 1)
      bool q2_brick = false;
      // a periodic axis (gls_mg_attach_periodic): its taps are stored unwrapped at the seam and the two-pass kernels
      // take their input modulo the lattice; never q2_brick, never the one-pass gather
      bool wrap = false;
    };
    std::vector<std::unique_ptr<Taps>> taps;
    // general hierarchies (gls_mg_attach_transfers): per level pair the prolongation P (fine rows), the
    // restriction R = P^T (coarse rows) as CSR, and the state injection (coarse DoF <- fine DoF)
    bool csr = false;
    bool ilu_smooth = false;  // gls_mg_params.smoother = 1: ILU(0) sweeps on the levels above the coarsest
    struct Csr {
      DevBuf<int64_t> poff, roff;
      DevBuf<int32_t> pcol, rcol, inj;
      DevBuf<double> pw, rw;
      int64_t nf = 0, nc = 0;
      int plane = 1, rlane = 1;  // SpMV lanes per row (from the mean row length)
    };
    std::vector<std::unique_ptr<Csr>> xfer;
    std::vector<gls_ctx *> ilu_levels;  // levels whose ILU(0) smoother this attach created (smoother = 1)
    DevBuf<double> xwork;  // two-pass transfer intermediate (coarse xy x fine z, 4 fields)
    // coarsest level: direct solve with the probed, regularised, factored Jacobian (gls_mg_coarse.hpp; coarse.ok:
    // this state's factorization stands)
    bool direct = false;
    // per-cell coarsest level: its matrix for the direct solve assembled by the ILU's colored batched probes
    // (a structure-only ILU(0) on that level, never factored) instead of one J.v per column
    gls_ctx *probe_ilu = nullptr;
    gls_impl::CoarseSolve coarse;
    // coarsest-level Jacobi sweeps (single rank, fused brick path) replayed as one HIP graph: the
    // ~2×csweeps tiny launches per V-cycle are captured once per state (mg_prepare) and launched
    // as a single graph by every V-cycle of that Newton step
    struct Graph {
      hipGraphExec_t h = nullptr;
      Graph() = default;
      Graph(const Graph &) = delete;
      Graph &operator=(const Graph &) = delete;
      Graph(Graph &&o) noexcept : h(o.h) { o.h = nullptr; }
      Graph &operator=(Graph &&o) noexcept {
        if (this != &o) {
          reset();
          h = o.h;
          o.h = nullptr;
        }
        return *this;
      }
      void reset() {
        if (h) (void)hipGraphExecDestroy(h);
        h = nullptr;
      }
      ~Graph() { reset(); }
    } cgraph;
    std::vector<unsigned char> cgraph_key;  // launch parameters the graph was captured with
    bool cgraph_failed = false;  // capture refused once: stay on plain launches
    bool dirty = true;
    // multi-GPU (gls_mg_set_coarse_replica): the coarsest DISTRIBUTED level's correction is computed
    // by a replica -- a single-rank context of that level's whole mesh with its own hierarchy below
    // it -- identically on every rank, from the all-reduced (gathered) right-hand side
    gls_ctx *replica = nullptr;
    // general hierarchies across ranks (gls_mg_attach_replica): the distributed fine level smooths its own
    // rows, every coarser level is a replica on every rank (rep2, with its own hierarchy); restriction over the
    // rank's OWNED fine rows into the replica numbering + a sum all-reduce, prolongation onto all local rows
    bool rep_csr = false;
    gls_ctx *rep2 = nullptr;
    DevBuf<int64_t> r2p_off, r2r_off;  // P (local fine rows x replica DoFs), R = P_owned^T (replica rows)
    DevBuf<int32_t> r2p_col, r2r_col;
    DevBuf<double> r2p_w, r2r_w;
    int r2p_lane = 1, r2r_lane = 1;
    DevBuf<int32_t> r2inj_c, r2inj_f;  // replica DoF <- owned local fine DoF (state injection pairs)
    DevBuf<int32_t> rep_own_loc, rep_own_glob;  // owned local rows of the coarsest level -> replica rows
    DevBuf<int32_t> rep_map;                    // every local row -> replica row
    DevBuf<double> rep_b, rep_x, rep_tmp, rep_u[4];
  } mg;
  double time_steps[4] = {1, 1, 1, 1};
  // frozen Jacobian (skip_newton: the matrix and its preconditioner are reused across Newton
  // iterations, skip_newton_non_linear_solver.h:66-70, 126-130): snapshot of the state and time
  // coefficients the Jacobian operators (J.v, diagonal, linearization, multigrid levels) are taken
  // at, while gls_set_state / gls_set_time move only the residual's state
  struct JacFreeze {
    bool on = false;
    DevBuf<double> u, h[3];
    bool has[3] = {false, false, false};
    double alpha[4] = {0, 0, 0, 0}, alpha_jac = 0., sdt2 = 0., ts[4] = {1, 1, 1, 1};
    int n_hist = 0, scheme = GLS_STEADY;
  } jf;
  int skip_consecutive = 0;  // SkipNewtonNonLinearSolver::consecutive_iters (persists across solves)
  bool probe_local = false;  // ILU probe across ranks: J.v on the rank's cells only (no ghost exchange)
  // TimerOutput sections of the reference's Newton/GMRES path (gls_section_timing): wall seconds and
  // calls, stream-synchronised at the section boundaries while enabled
  bool sec_on = false;
  double sec_t[GLS_N_SECTIONS] = {};
  int sec_n[GLS_N_SECTIONS] = {};
  // timing
  bool timing = false;
  struct Ev { int which; hipEvent_t a, b; };
  std::vector<Ev> events;
  // residual, J.v, diagonal, J.v linearization, FP32 smoother J.v, brick-surface slab sums
  double t_ms[6] = {0, 0, 0, 0, 0, 0};
  int64_t t_n[6] = {0, 0, 0, 0, 0, 0};

  ~gls_ctx() {
    if (hpin) (void)hipHostFree(hpin);
    for (auto &e : events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (dist.ev_ready) (void)hipEventDestroy(dist.ev_ready);
    if (dist.ev_done) (void)hipEventDestroy(dist.ev_done);
    if (dist.xstream) (void)hipStreamDestroy(dist.xstream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

namespace gls_impl {

// ---- gls_api.cpp
inline int check_ctx(gls_ctx *c) {
  if (!c) return set_err(GLS_EINVAL, "null context");
  return GLS_OK;
}

// jac: parameters of the Jacobian operators (the frozen snapshot when gls_freeze_jacobian is on)
gls::OpParams make_params(gls_ctx *c, bool jac = false);

struct TimedLaunch {
  gls_ctx *c;
  int which;
  hipEvent_t a = nullptr, b = nullptr;
  TimedLaunch(gls_ctx *c_, int w) : c(c_), which(w) {
    if (c->timing) {
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      (void)hipEventRecord(a, c->stream);
    }
  }
  ~TimedLaunch() {
    if (c->timing) {
      (void)hipEventRecord(b, c->stream);
      c->events.push_back({which, a, b});
    }
  }
};

// QGauss(n) and the FE_Q support points (Gauss-Lobatto) on [0,1]; Lagrange basis i on nodes xn: value, first and
// second derivative at s
void gauss_points(int n, double *x, double *w);
void lobatto_points(int k, double *x);
void lagrange_1d(int k, const double *xn, int i, double s, double &v, double &d, double &dd);
// cell->measure() of a mapped cell from its corner support points
double corner_measure(int dim, int md, const double *S);
// slots of every node in the per-cell element vectors (built on first use)
int ensure_element_maps(gls_ctx *c);
// the Jacobian's diagonal at the current state
int ensure_diag(gls_ctx *c);
// the per-cell linearization cache: on for contexts that run the per-cell kernels
inline bool cell_cache_on(const gls_ctx *c) {
  return !c->use_brick && c->n_cells > 0;
}
inline size_t cell_cache_size(const gls_ctx *c) {
  const int dim = c->dim;
  return (size_t)c->n_cells * (size_t)gls::ipow(c->nq1d, dim) * (size_t)(dim + dim * dim + 1 + dim);
}

// brick launch output: the slab (allocated on first use) or nullptr (atomics into a zeroed y)
double *brick_slab(gls_ctx *c);
// distributed hooks (no-ops on a single rank): ghost values imported into x; ghost rows' sums export-added into y;
// in-place sum over ranks of a device vector
int dist_import(gls_ctx *c, double *x);
int dist_export_add(gls_ctx *c, double *y);
int dist_allreduce_vector(gls_ctx *c, double *v, int64_t n);
// the brick J.v's linearization at the quadrature points, once per state; its FP32 copy (full = false: u and tau
// suffice, the Oseen smoother operator)
int ensure_qdata(gls_ctx *c);
int ensure_qdata32(gls_ctx *g, bool full = true);
// FP32 kernels write their brick-surface partial sums in FP32
bool slab_f32();
// the V-cycle's operator and sweeps on level g (mixed precision and the Oseen operator per gls_mg_params):
// y = A v, or y = rb - A v; first_omega > 0 (only where first_sweep_fusable): v formed as the first damped-Jacobi
// sweep from 0 inside the J.v
bool first_sweep_fusable(gls_ctx *g);
int jacobian_apply_f32(gls_ctx *g, const double *v, double *y, const double *rb = nullptr, double first_omega = 0.0,
                       bool oseen = false);
int smoother_apply(gls_ctx *g, const double *v, double *y, const double *rb = nullptr);
// one smoothing sweep on x: damped Jacobi, or the level's ILU(0) when z (scratch) is given and it is attached;
// pxc != nullptr (only where the prolongation fuses): the sweep starts from x + P pxc
int smoother_sweep(gls_ctx *g, double *x, const double *b, double *y, double omega, double *z = nullptr,
                   const double *pxc = nullptr);

// ---- gls_mg.cpp: the geometric multigrid. mg_prepare re-discretises the levels at the Jacobian's state and factors
// the coarsest one (no-op unless the state changed); x = V-cycle(b) on level l, and with the replica hierarchy below
// a distributed fine level (gls_mg_attach_replica). x0_ready: x already holds the level's first damped-Jacobi sweep
// from 0 (stored by the kernel that wrote b), which the cycle then does not launch
int mg_prepare(gls_ctx *c);
int mg_vcycle(gls_ctx *c, int l, const double *b, double *x, bool x0_ready = false);
int mg_vcycle_rep2(gls_ctx *c, const double *b, double *x);
// *d = level 0's diagonal and *omega its damping when mg_vcycle(c, 0, b, x, true) honours x0_ready, else nullptr
int mg_fine_first_producer(gls_ctx *c, const double **d, double *omega);

// ---- gls_ilu.cpp: the assembled ILU (probe the operator into the CSR values; probe + perturb + factor once per
// Jacobian state; z = P^T U^-1 L^-1 P v)
int ilu_probe(gls_ctx *c);
int ensure_ilu(gls_ctx *c);
int apply_ilu(gls_ctx *c, const double *v, double *z);

// ---- gls_vanka_host.cpp: the additive cell-Vanka smoother. vanka_refusal: nullptr, or why the context cannot carry it;
// vanka_attach builds the maps (no-op when on); ensure_vanka rebuilds the inverses when the linearization changed;
// one sweep x <- x + omega D_m^-1 sum_c R_c^T A_c^-1 R_c (b - A x) (y: scratch; x_zero: x is taken as 0 and set)
const char *vanka_refusal(const gls_ctx *c);
int vanka_attach(gls_ctx *c);
int ensure_vanka(gls_ctx *c);
int vanka_sweep(gls_ctx *c, double *x, const double *b, double *y, double omega, bool x_zero = false);

// ---- gls_rccl.cpp: the RCCL transport's exchange on a given stream
int rccl_exchange_on(gls_ctx *c, int phase, hipStream_t stream);

}  // namespace gls_impl
