/* gls_native.h — C-ABI of the MI355X-native GLS Navier–Stokes hot path.
 *
 * Drop-in boundary for Lethe's GLSNavierStokesSolver assembly + linear-solve path.
 * Every entry point below names the reference interface it replaces
 * (paths relative to the reference tree, LMNS3d/SOFTX_2020_200).
 *
 * Conventions
 *   - Plain C types only: pointers, sizes, doubles. No torch / HIP types in signatures
 *     (streams are passed as void*; NULL = the context's own stream).
 *   - Return 0 on success or a negative GLS_E* code; gls_last_error() gives the text
 *     (thread-local). No C++ exception ever crosses this boundary
 *     (the reference throws std::runtime_error, gls_navier_stokes.cc:825, :1158).
 *   - Vectors are FP64, global layout [velocity node-major, comps interleaved | pressure]:
 *       dof(vnode, c) = vnode*dim + c,  dof(pnode) = dim*n_vnodes + pnode.
 *   - Operator entry points take DEVICE pointers (hipMalloc / torch cuda tensors); calls are
 *     stream-ordered on the context stream. Host-pointer entry points say so.
 *   - One context per GPU; the multi-GPU context (gls_dist_*) wraps RCCL.
 */
#ifndef GLS_NATIVE_H
#define GLS_NATIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLS_OK 0
#define GLS_EINVAL -1   /* bad argument / unsupported configuration */
#define GLS_EHIP -2     /* HIP runtime error */
#define GLS_ENOMEM -3   /* device allocation failed */
#define GLS_ENOCONV -4  /* linear solver did not converge (informational) */
#define GLS_EIO -5      /* file / parse error */
#define GLS_ECOMM -6    /* RCCL error */
#define GLS_ENOTFOUND -7 /* parameter entry absent (gls_prm_get; the caller applies the default) */

/* TimeSteppingMethod, same order as include/core/parameters.h:56-69 */
enum gls_scheme {
  GLS_STEADY = 0, GLS_BDF1, GLS_BDF2, GLS_BDF3, GLS_SDIRK2, GLS_SDIRK2_1, GLS_SDIRK2_2,
  GLS_SDIRK3, GLS_SDIRK3_1, GLS_SDIRK3_2, GLS_SDIRK3_3
};

const char *gls_last_error(void);
const char *gls_version(void);

/* ------------------------------------------------------------------------------------------
 * Mesh / DoF map description (host pointers, copied at gls_create).
 * Replaces NavierStokesBase ctor FESystem(FE_Q(k)^dim, FE_Q(kp)) + QGauss(k+1)
 * (source/solvers/navier_stokes_base.cc:62,70) and GLSNavierStokesSolver::setup_dofs
 * (source/solvers/gls_navier_stokes.cc:55-228): cell->DoF map, zero_constraints mask.
 * Cells are axis-aligned boxes (hyper_cube / subdivided meshes, MappingQ affine on them).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int dim;                      /* 2 or 3 */
  int k;                        /* velocity degree (1..3) */
  int kp;                       /* pressure degree (1..k) */
  int nq1d;                     /* QGauss points per direction, 0 = k+1 (navier_stokes_base.cc:70, :93-94) */
  int n_cells;
  int n_vnodes, n_pnodes;
  const int32_t *cell_vnodes;   /* [n_cells*(k+1)^dim], lexicographic local node order (x fastest) */
  const int32_t *cell_pnodes;   /* [n_cells*(kp+1)^dim]; NULL when kp==k and pressure nodes == velocity nodes */
  const double *cell_x0;        /* [n_cells*dim] lower corner (used by the SRF source term); may be NULL */
  const double *cell_h;         /* [n_cells*dim] extents */
  const uint8_t *vnode_mask;    /* [n_vnodes] bit c set = velocity comp c is in zero_constraints; NULL = none */
  double viscosity;             /* physical properties/kinematic viscosity */
  int srf;                      /* velocity source = srf (parameters.h:511-515) */
  double omega[3];
  const double *force_q;        /* [n_cells*nq*dim] forcing at quadrature points; NULL = NoForce */
  /* General (curved / unstructured) cells: MappingQ(map_degree) of FEValues (gls_navier_stokes.cc:
   * 245-252). 0 = axis-aligned boxes given by cell_x0 / cell_h (the brick fast path). > 0: the
   * cells' mapping support points, lexicographic on the equidistant (map_degree+1)^dim lattice
   * (Q1 cells of a MappingQ(k, qmapping_all = false) mesh are passed as their exact Qk embedding).
   * Jacobians, JxW, the Hessian mapping correction and the quadrature points are derived per
   * quadrature point at gls_create; cell->measure() (h of tau) from the cell's corner vertices. */
  int map_degree;
  const double *cell_support;   /* [n_cells][(map_degree+1)^dim][dim] */
} gls_mesh_desc;

typedef struct gls_ctx gls_ctx;

/* setup_dofs equivalent: uploads the DoF map, geometry, tabulated 1D bases. */
int gls_create(const gls_mesh_desc *desc, gls_ctx **out);
int gls_destroy(gls_ctx *ctx);
int gls_set_stream(gls_ctx *ctx, void *hip_stream);
int gls_n_dofs(const gls_ctx *ctx, int64_t *n_dofs);
/* Physical quadrature points QGauss(nq1d) of every cell (HOST array [n_cells][nq][dim]): where the
 * caller evaluates forcing (gls_set_force) and analytical functions; the mapped points for
 * general cells. */
int gls_quadrature_points(const gls_ctx *ctx, double *xq);
/* 1 when the context runs the sum-factorized brick kernels (3D Qk-Qk on Morton 2x2x2 bricks),
 * 0 for the general per-cell kernels. GLS_DISABLE_BRICK=1 in the environment forces 0. */
int gls_uses_brick_kernels(const gls_ctx *ctx);
/* How the context sums the bricks' surface slab: 0 through the node -> slot index map (or not at all: no brick
 * kernels), 1 by the closed form of the verified hyper_cube (Morton bricks), 2 by the closed form of the verified open
 * subdivided hyper_rectangle (tile-Morton bricks, gls_mesh_hyper_rectangle). nb[3] (bricks per axis) and tile (bricks
 * per tile edge; the cube: its brick count) are set for 1 and 2; either may be NULL. */
int gls_slab_lattice(const gls_ctx *ctx, int nb[3], int *tile);
/* Rewrite the forcing at quadrature points (host pointer, [n_cells*nq*dim]) or clear it (NULL). */
int gls_set_force(gls_ctx *ctx, const double *force_q);
int gls_set_viscosity(gls_ctx *ctx, double viscosity);

/* Time-stepping state for the next assembly (replaces the top of assembleGLS,
 * gls_navier_stokes.cc:295-329: time_steps_vector -> bdf_coefficients / sdirk_coefficients). */
int gls_set_time(gls_ctx *ctx, int scheme, const double time_steps[4]);

/* Evaluation point and history (DEVICE pointers, borrowed until the next call):
 * evaluation_point, solution_m1..m3 of PhysicsSolver (include/core/physics_solver.h:107-111).
 * u1..u3 may be NULL when the scheme does not read them. The state is captured here: the
 * Jacobian diagonal and the J.v linearization (per quadrature point) are cached until the next
 * gls_set_state / gls_set_time / gls_set_viscosity / gls_set_force, so changing the vectors'
 * contents in place requires calling gls_set_state again. */
int gls_set_state(gls_ctx *ctx, const double *u, const double *u1, const double *u2, const double *u3);

/* assemble_rhs (gls_navier_stokes.cc:1023-1128 -> assembleGLS<false,...>):
 * rhs = -R(u) with zero_constraints (constrained rows 0). DEVICE pointer, length n_dofs. */
int gls_residual(gls_ctx *ctx, double *rhs);

/* Matrix-free action of the reference's assembled Jacobian (assembleGLS<true,...>,
 * gls_navier_stokes.cc:519-625, distributed with zero_constraints :758-765):
 * Jv = P J P v + D_c v, D_c = sum over cells of |local(i,i)| on constrained DoFs (deal.II rule).
 * Replaces system_matrix.vmult inside Trilinos GMRES (gls_navier_stokes.cc:1276-1279). */
int gls_jacobian_apply(gls_ctx *ctx, const double *v, double *Jv);

/* The same operator evaluated in FP32 arithmetic from an FP32 copy of the linearization (3D
 * Qk-Qk brick path only; v, Jv are FP64 DEVICE vectors): the operator the mixed-precision
 * multigrid V-cycle smooths with (gls_mg_params.mixed_precision). Not a reference interface: a
 * preconditioner-internal operator, exposed for parity tests (relative error ~1e-6). */
int gls_jacobian_apply_f32(gls_ctx *ctx, const double *v, double *Jv);

/* Hanging-node constraints (DoF level), after the Dirichlet mask of gls_create:
 *   DoF dofs[i] = sum_{j in [offsets[i], offsets[i+1])} weights[j] * DoF masters[j]
 * (DoFTools::make_hanging_node_constraints, gls_navier_stokes.cc:84, 143; host arrays). Hanging
 * DoFs must not carry a Dirichlet mask bit (deal.II: interpolate_boundary_values skips DoFs that
 * are already constrained) and may not be masters; Dirichlet masters drop out of the operators
 * (closed zero_constraints). The operators then are those of the reference's condensed system
 * (AffineConstraints::distribute_local_to_global): residual and J.v rows of hanging DoFs are
 * condensed onto their masters, the hanging rows themselves are 0 / D_c v; gls_apply_dirichlet
 * also distributes the hanging values (nonzero_constraints.distribute). The diagonal returned by
 * gls_jacobian_diagonal stays the element-diagonal sum on unconstrained rows (a Jacobi scaling,
 * not the condensed diagonal). Single GPU, per-cell kernels (no bricks, no multigrid). */
int gls_set_hanging(gls_ctx *ctx, int64_t n_lines, const int64_t *dofs, const int64_t *offsets,
                    const int64_t *masters, const double *weights);

/* Adapted forests (after gls_set_hanging on 3D Q2-Q2 box cells): the number of complete sibling groups
 * of leaves (8 consecutive cells forming a 2x2x2 brick) whose J.v / diagonal run the sum-factorised pencil
 * kernel (cached linearization, element-vector output summed with the per-cell kernel's); 0 = per-cell
 * kernels only (GLS_OCT_BRICKS=0 in the environment forces it). */
int gls_forest_bricks(const gls_ctx *ctx);

/* Diagonal of that assembled Jacobian (DEVICE pointer). */
int gls_jacobian_diagonal(gls_ctx *ctx, double *diag);

/* assemble_matrix_and_rhs (gls_navier_stokes.cc:917-1000, assembleGLS<true>: the matrix and the rhs in
 * one pass over the cells): the residual into rhs (as gls_residual) and the Jacobian's diagonal (as
 * gls_jacobian_diagonal; diag may be NULL) at the current state, with the J.v linearization cached.
 * On the 3D Q2 brick path one fused launch computes all three; the values equal those of the separate
 * calls bitwise. DEVICE pointers. */
int gls_residual_and_diagonal(gls_ctx *ctx, double *rhs, double *diag);

/* Apply nonzero_constraints.distribute to a DEVICE vector: x[dof] = value for listed DoFs
 * (PhysicsSolver::apply_constraints, physics_solver.h:98-102). Host arrays, copied. */
int gls_set_dirichlet(gls_ctx *ctx, int64_t n, const int64_t *dofs, const double *values);
int gls_apply_dirichlet(gls_ctx *ctx, double *x);

/* ------------------------------------------------------------------------------------------
 * Linear solve: replaces solve_system_GMRES + setup_ILU (gls_navier_stokes.cc:1242-1289,
 * :1161-1176). Right-preconditioned restarted GMRES on the matrix-free operator with a
 * Jacobi (diagonal) preconditioner; tolerance = max(rel*||rhs||, abs) as the reference.
 * x and rhs are DEVICE pointers. Returns GLS_OK or GLS_ENOCONV (x holds the last iterate).
 * ------------------------------------------------------------------------------------------ */
#define GLS_LIN_GMRES 0     /* solve_system_GMRES (gls_navier_stokes.cc:1242-1289) */
#define GLS_LIN_BICGSTAB 1  /* solve_system_BiCGStab (gls_navier_stokes.cc:1293-1340): right-preconditioned
                               BiCGStab, same preconditioner and tolerance rule; an iteration = one
                               BiCGStab step (two operator applications), as AztecOO counts them */
#define GLS_ORTHO_GRAM 0    /* GMRES: Gram-corrected single-pass classical Gram-Schmidt (default) */
#define GLS_ORTHO_CGS2 1    /* GMRES: classical Gram-Schmidt + DGKS re-orthogonalisation pass */
typedef struct {
  int max_iterations;     /* linear solver/max iters */
  int restart;            /* GMRES restart (deal.II default 30) */
  double relative_residual, minimum_residual;
  int iterations;         /* out */
  double final_residual;  /* out */
  int method;             /* GLS_LIN_GMRES (0, default) | GLS_LIN_BICGSTAB ('linear solver/method',
                             parameters.cc:519-532; 'amg' is GMRES with the caller's preconditioner) */
  int orthogonalization;  /* GMRES only: GLS_ORTHO_GRAM (0) | GLS_ORTHO_CGS2 */
  int true_residual;      /* in: 1 = on convergence recompute ||b - A x|| into final_residual (one extra
                             operator application); 0 = the Krylov recurrence estimate (deal.II) */
} gls_linear_params;
int gls_solve_linear(gls_ctx *ctx, const double *rhs, double *x, gls_linear_params *prm);

/* Geometric multigrid preconditioner (matrix-free, monolithic), replacing the Jacobi default of
 * gls_solve_linear (the reference's ILU / ML-AMG setup, gls_navier_stokes.cc:1161-1240).
 * levels[0] = ctx; levels[l] = caller-created contexts of the same problem on the nested
 * hyper_cube with n/2^l cells per direction (same k, same boundary conditions and Dirichlet
 * lists). Each V-cycle: damped-Jacobi smoothing with the level's own matrix-free GLS Jacobian at
 * the injected state, exact Qk restriction/prolongation. 3D Q1-Q1 / Q2-Q2. The coarse levels are
 * switched to ctx's stream (and follow later gls_set_stream calls on ctx).
 * Multi-GPU: every level is a distributed context (gls_dist_attach on the partition of its own
 * hyper_cube; nested partitions: rank r's coarse cells are the parents of its fine cells) that
 * also declared its lattice embedding with gls_set_lattice. Restriction sums owned fine rows and
 * export-adds the coarse ghost rows; prolongation imports the coarse ghosts first. */
typedef struct {
  int n_levels;
  gls_ctx **levels;
  int pre_smooth, post_smooth, coarse_sweeps;  /* pre: 0 -> 2, < 0 -> none (x = 0, residual = rhs);
                                                  post: < 0 -> 2, 0 -> none; coarse: 0 -> 30 */
  double omega;                               /* damped-Jacobi weight of the smoother, 0 -> 0.6
                                                 (smoother 3: the cell-Vanka damping, 0 -> 0.8) */
  double coarse_omega;                        /* weight of the coarsest-level Jacobi sweeps, 0 -> omega
                                                 (smoother 3: 0 -> 0.6 whatever omega is) */
  int coarse_direct;                          /* coarsest level: 0 auto (exact solve when on one GPU
                                                 with <= 2048 DoFs), 1 direct solve (<= 40000 DoFs;
                                                 a gls_mg_attach_replica level <= 8192),
                                                 -1 Jacobi sweeps. The direct solve probes the coarsest
                                                 Jacobian and factors it by rocSOLVER LU with the
                                                 first pressure DoF pinned (the enclosed-flow gauge).
                                                 Up to 8192 DoFs FP64: unpivoted by default, the
                                                 inverse checked by max|A (A^-1 e) - e| and finiteness;
                                                 a zero pivot or a failed check refactors with partial
                                                 pivoting (GLS_MG_COARSE_SOLVER=lu: always pivoted).
                                                 Above: FP32 unpivoted (sgetrf_npvt by a library worker
                                                 thread on a side stream, overlapping the finer levels'
                                                 setup), applied by blocked triangular solves; checked
                                                 by |A x - 1| / |1|: < 1e-2 as it is, < 0.5 with one
                                                 refinement step against the FP64 matrix, else pivoted
                                                 FP32 LU + explicit inverse.
                                                 1 above 40000 DoFs, or 2 at any size: the band route
                                                 (gls_band_lu_* below) -- the FP32 matrix in block-
                                                 tridiagonal storage filled from the probing ILU's CSR,
                                                 no n x n array; same check and refinement against the
                                                 FP64 CSR, no pivoted fallback (a failed check is
                                                 GLS_EINVAL at the first coarse solve and the hierarchy
                                                 prepares again). It needs a coarsest level probed
                                                 through its ILU CSR (a per-cell context without an ILU
                                                 or hierarchy of its own, gls_mg_attach_transfers;
                                                 not a gls_mg_attach_replica level) whose panels plus CSR take at most half of
                                                 the free device memory at attach (or
                                                 GLS_MG_BAND_MAX_BYTES, if less); else GLS_EINVAL
                                                 (a brick or column-probed level: before anything is
                                                 detached). GLS_MG_VERBOSE prints a `band storage` line */
  int mixed_precision;                        /* 1: the V-cycle's smoothing / residual J.v run in FP32
                                                 arithmetic from an FP32 copy of the linearization
                                                 (brick path; vectors, transfers and the outer GMRES
                                                 operator stay FP64). 0: all FP64 (an FP32 copy of the
                                                 ILU smoothers' factors measured slower:
                                                 profiles/r06_ab_ilu_fp32_factors.txt) */
  const int *level_sweeps;                    /* optional (NULL: uniform): 2*n_levels ints, the
                                                 pre / post sweep counts of each level (the entries of
                                                 the coarsest level are ignored) */
  int smoother;                               /* 0: damped Jacobi (omega); 1: ILU(0) of each level's
                                                 probed Jacobian, undamped (the smoother Trilinos ML
                                                 uses under the reference's AMG, gls_navier_stokes.cc:
                                                 1208-1226); levels with hanging nodes only
                                                 (gls_mg_attach_transfers); 2: ILU(0) on the coarser
                                                 levels, damped Jacobi on the finest (its FP32 brick
                                                 J.v with mixed_precision); 3: additive cell-Vanka on
                                                 every level above the coarsest (gls_mg_attach_transfers
                                                 on one rank; see gls_vanka_sweep): one sweep is
                                                 x += omega D_m^-1 sum_c R_c^T A_c^-1 R_c (b - A x)
                                                 with the dense inverse of the assembled Jacobian on
                                                 each cell's DoFs, averaged by the number of cells
                                                 holding a DoF; omega 0 -> 0.8. No probed CSR, no
                                                 colouring; the inverses are rebuilt once per Jacobian
                                                 state. 3D Q2-Q1 / Q2-Q2 per-cell contexts (mapped or
                                                 box cells) without hanging / slip lines; else
                                                 GLS_EINVAL and the context keeps what it had */
  int smoother_operator;                      /* 0: the levels' Newton Jacobian; 1: its Oseen (Picard)
                                                 linearization on the FP32 brick levels (no (grad u) v
                                                 terms, no SUPG tau (v . grad phi) R_s term): cheaper
                                                 smoothing J.v; the outer GMRES operator is the exact
                                                 Jacobian either way */
} gls_mg_params;
int gls_mg_attach(gls_ctx *ctx, const gls_mg_params *prm);
/* The same hierarchy on hyper_cubes with periodic directions (bit d of periodic_mask: direction d is periodic;
 * mask 0 is gls_mg_attach). Level l has n_l = cbrt(n_cells) cells per direction, n_{l+1} = n_l / 2, and its Qk node
 * lattice has k n_l nodes on a periodic axis and k n_l + 1 on the others, so nf = 2 nc across a periodic axis and
 * nf = 2 nc - 1 elsewhere. Every level's node numbering is checked cell by cell against the lexicographic wrapped
 * lattice of gls_mesh_hyper_cube(..., periodic_mask, ...) (any cell order). The interpolation is the open lattice's
 * without the clamp at the far end: fine node i lies in coarse cell floor(i / (2k)) and coarse node (cc k + q) mod nc
 * carries the weight; restriction is the transpose (Q2: every coarse vertex node has the full five-tap row). The
 * transfers run the two-pass kernels, which wrap at the seam where they load; the restriction / prolongation fused
 * into the smoother launches (gls_mg_residual_restrict, gls_mg_prolong_smooth) are the open cube's, so periodic
 * levels report fused = 0. GLS_EINVAL with a message, before anything is detached (the context keeps the hierarchy
 * it had): a level that is not that lattice (the level is named), a distributed context or level with a non-zero
 * mask, a level with fewer than 2 cells per direction, and whatever gls_mg_attach refuses. One GPU. */
int gls_mg_attach_periodic(gls_ctx *ctx, const gls_mg_params *prm, int periodic_mask);
/* The same hierarchy on subdivided hyper_rectangles (gls_mesh_hyper_rectangle): level l has cells[a] >> l cells on
 * axis a, every count even on every level (the coarsest included: the levels are brick meshes), at least 2 cells on
 * an open axis and 4 on a periodic one. Every level, mask 0 included, is checked cell by cell against the wrapped
 * lexicographic lattice of its counts (any cell order); nf = 2 nc - 1 across an open axis and 2 nc across a periodic
 * one, tap tables and two-pass transfers as in gls_mg_attach_periodic. The transfers fused into the smoother launches
 * stay the open cube's: cells = (n, n, n) with mask 0 is gls_mg_attach, with a mask gls_mg_attach_periodic (the same
 * transfers and V-cycle, bitwise); every other box reports fused = 0. GLS_EINVAL with a message naming the level and
 * the axis, before anything is detached (the context keeps the hierarchy it had): an odd count, too few cells, a
 * level whose cell count or numbering is not that lattice, a distributed context or level, and whatever
 * gls_mg_attach refuses. One GPU. */
int gls_mg_attach_box(gls_ctx *ctx, const gls_mg_params *prm, const int cells[3], int periodic_mask);
/* The same V-cycle on a general level hierarchy with the caller's grid transfers: levels of an adaptive
 * (octree) mesh with hanging-node constraints (gls_set_hanging before attaching), e.g. the global
 * coarsening gls_octree_coarsen_to / gls_octree_mg_transfer builds. For l = 0 .. n_levels-2:
 * p_off[l] (n_dofs(l)+1), p_col[l], p_w[l] = the prolongation from level l+1 to level l as CSR (rows of
 * constrained fine DoFs may be empty), inject[l] (n_dofs(l+1)) = the level-l DoF whose value the
 * level-(l+1) state takes (hanging values are then distributed from their lines). Restriction = P^T;
 * the V-cycle zeroes constrained rows (Dirichlet and hanging) after each transfer. Smoothing: damped
 * Jacobi with each level's own operator (per-cell kernels on hanging levels, FP64). One GPU. Host arrays
 * (copied). The levels may differ in element degree (h-p hierarchies: a Q2-Q1 level above Q1-Q1 ones, the
 * p-level pairs of gls_fe_space_mg_transfer), not in dimension. */
int gls_mg_attach_transfers(gls_ctx *ctx, const gls_mg_params *prm, const int64_t *const *p_off,
                            const int32_t *const *p_col, const double *const *p_w, const int64_t *const *inject);
/* The refinement-hierarchy V-cycle ACROSS RANKS on general meshes (the reference's AMG is global,
 * gls_navier_stokes.cc:1180-1240): ctx is the rank-local fine context (distributed with
 * gls_dist_attach_dofs[_rccl]); every coarser level runs as a REPLICA on every rank: `replica` is a
 * single-rank context of the level-1 mesh (the whole of it) with its own hierarchy attached (e.g.
 * gls_mg_attach_transfers), so the N-rank V-cycle is the one-rank V-cycle up to the fine level's smoother.
 * p_off (n_local + 1) / p_col / p_w: the prolongation from level 1 (replica DoFs) onto the rank's local fine
 * DoFs, owned and ghost rows; inject (replica n_dofs): the local fine DoF whose value the replica's state
 * takes, on the one rank that owns it (-1 elsewhere). The restriction sums P^T over each rank's owned rows
 * and all-reduces in the replica numbering. prm: pre / post smooth, omega, smoother (0 damped Jacobi, 1
 * ILU(0) per rank = Ifpack additive Schwarz, overlap 0; the cell-Vanka smoother 3 is one-rank: GLS_EINVAL); coarse_direct > 0 with a replica WITHOUT a hierarchy
 * of its own (two-level case): the replica level is solved exactly (probed, LU-inverted, <= 8192 DoFs) on
 * every rank; levels / other coarse entries are not used. Host arrays. */
int gls_mg_attach_replica(gls_ctx *ctx, const gls_mg_params *prm, gls_ctx *replica, const int64_t *p_off,
                          const int32_t *p_col, const double *p_w, const int64_t *inject);
/* The attached hierarchy's direct coarse solve: *n its unknowns (0: none, the coarsest level is smoothed), *storage 0
 * dense arrays, 1 band storage; bl / bu / nb the band route's bandwidths and block width (-1 otherwise), *bytes the
 * matrix storage held (dense: the FP64 array plus the FP32 one above 8192 DoFs; band: the panels). Any output may be
 * NULL. */
int gls_mg_coarse_info(gls_ctx *ctx, int64_t *n, int *storage, int64_t *bl, int64_t *bu, int64_t *nb, int64_t *bytes);
/* z = M^-1 v with the preconditioner gls_solve_linear uses at the current state (the V-cycle when
 * attached, else Jacobi): the reference's preconditioner vmult (DEVICE pointers, no aliasing). */
int gls_apply_preconditioner(gls_ctx *ctx, const double *v, double *z);
/* y = A_s v: the operator the attached V-cycle smooths this level with (the Jacobian, in FP32 with
 * gls_mg_params.mixed_precision, its Oseen part with smoother_operator = 1); DEVICE pointers. */
int gls_mg_smoother_apply(gls_ctx *ctx, const double *v, double *y);
/* Multigrid grid transfer between levels `level` and `level`+1 of the attached hierarchy (DEVICE
 * pointers): direction 0 restricts a level-`level` vector into level `level`+1 (transpose of the
 * Qk interpolation, the reference's MGTransfer restrict_and_add into a zeroed vector), direction 1
 * prolongates a level-`level`+1 vector onto level `level` (exact Qk interpolation). Constrained
 * rows are not touched here; the V-cycle zeroes them. */
int gls_mg_transfer(gls_ctx *ctx, int level, int direction, const double *in, double *out);
/* Debug / test entry: the coarse right-hand side the V-cycle forms on level `level`+1 from level `level`'s
 * iterate x and right-hand side b at the current state, bc = R (b - A_s x) with the constrained coarse
 * rows zeroed (DEVICE pointers; x, b: level `level` vectors, bc: level `level`+1). Where the level is
 * eligible (one rank, FP32 smoothing on the hyper_cube's Q2 bricks, nested lattice levels) the residual
 * is restricted inside the smoother's J.v launch and summed on the coarse lattice; else, or with
 * GLS_MG_FUSE_TRANSFER=0 / GLS_MG_NO_FUSE in the environment, by the separate residual, transfer and
 * zeroing launches. *fused (may be NULL) reports which of the two ran. */
int gls_mg_residual_restrict(gls_ctx *ctx, int level, const double *x, const double *b, double *bc, int *fused);
/* Debug / test entry: the V-cycle's prolongation and first post-sweep on level `level` at the current state,
 * x <- S(x + P xc) with one damped-Jacobi (or ILU) sweep S of damping omega >= 0 for the right-hand side b (DEVICE
 * pointers; x, b: level `level` vectors, x updated in place; xc: level `level`+1). Where the level pair is eligible
 * (one rank, FP32 smoothing with the fused Jacobi sweep on the hyper_cube's Q2 bricks, nested lattice levels,
 * at least one post-sweep) the coarse correction is interpolated inside the sweep's J.v and slab-sum launches;
 * else, or with GLS_MG_FUSE_PROLONG=0 / GLS_MG_NO_FUSE in the environment, by the separate transfer launches
 * before the sweep. *fused (may be NULL) reports which of the two ran. */
int gls_mg_prolong_smooth(gls_ctx *ctx, int level, const double *xc, double *x, const double *b, double omega,
                          int *fused);
/* Lattice embedding of a (rank-local) mesh: its velocity nodes are a subset of the global n1d^3
 * Qk node lattice of hyper_cube in canonical numbering (global id = x + n1d*(y + n1d*z)), local
 * node i being global node local_to_global[i] (host array, n_vnodes entries). The local nodes
 * must fill an axis-aligned box (Morton partitions of a 2^m-cube over 2^j ranks do). */
int gls_set_lattice(gls_ctx *ctx, int n1d, const int64_t *local_to_global);
int gls_mg_detach(gls_ctx *ctx);
/* Multi-GPU: the V-cycle below the coarsest DISTRIBUTED level is the single-GPU one, computed
 * redundantly on every rank. replica = a single-rank context of that level's WHOLE mesh (same problem
 * and boundary data) with its own gls_mg_attach hierarchy below it (e.g. the exact LU level of the
 * one-GPU cycle); local_to_replica[i] = the replica row of the coarsest level's local row i (n_local =
 * its n_dofs). The coarsest level's correction becomes: all-reduce its owned right-hand-side rows into
 * the replica numbering, apply the replica's preconditioner, take back the local rows. Its state, time
 * data and viscosity follow the hierarchy's (gathered at every Jacobian state). With the replica the
 * N-rank cycle performs the operations of the 1-rank cycle (bench.py --gpus N). */
int gls_mg_set_coarse_replica(gls_ctx *ctx, gls_ctx *replica, int64_t n_local, const int64_t *local_to_replica);
/* Additive cell-Vanka smoother (gls_mg_params.smoother = 3) and its building blocks, each callable on a context
 * without a hierarchy (tests, experiments). Not a reference interface: the reference smooths with Trilinos ML's ILU.
 * Supported: 3D Q2-Q1 / Q2-Q2 contexts on the per-cell kernels (mapped or box cells), one rank, no hanging-node or
 * slip lines, no forest context whose sibling groups run the brick (pencil) kernel (gls_forest_bricks > 0), no cell
 * that holds a node twice (periodic identification across one cell; a periodic mesh in which no cell meets itself is a
 * conforming mesh to the patches and is supported); anything else returns GLS_EINVAL with the limit named. nd = 81 + (kp+1)^3 DoFs per cell in the element-vector order (velocity
 * node a, component c at 3 a + c; pressure node b at 81 + b). DEVICE pointers unless said otherwise.
 *   gls_vanka_sizes            : nd and the padded row length (floats, a multiple of 4) of the FP32 inverses.
 *   gls_vanka_element_matrices : K [n_cells][nd][nd] row-major, the cells' local Jacobians at the current (or frozen)
 *                                state, unconstrained: the matrix local_matrix of assembleGLS<true> holds
 *                                (gls_navier_stokes.cc:519-625), from the J.v linearization cache.
 *   gls_vanka_patch_inverses   : rebuilds (when the Jacobian's state changed) and copies out A [n_cells][nd][nd], the
 *                                assembled Jacobian gls_jacobian_apply applies restricted to each cell's DoFs
 *                                (constrained DoFs: identity rows / columns times D_c), and / or Ainv
 *                                [n_cells][nd][row floats], its FP32 inverse (FP64 Gauss-Jordan with partial pivoting);
 *                                either may be NULL. The library keeps A across rebuilds only after a call that asked
 *                                for it (2 nd^2 doubles per cell; the smoother needs the inverses alone). A singular
 *                                or non-finite patch: GLS_EINVAL naming the first cell.
 *   gls_vanka_sweep            : x <- x + omega D_m^-1 sum_c R_c^T A_c^-1 R_c (b - A x) (omega <= 0 -> 0.8); the
 *                                residual in FP64 by gls_jacobian_apply, the patch products in FP32, sums in a fixed
 *                                order (bitwise repeatable).
 *   gls_vanka_detach           : releases the maps, matrices and inverses (gls_mg_detach does it for the levels a
 *                                hierarchy smoothed).
 *   gls_vanka_maps             : HOST only, no device: the maps the patches are assembled with. cell_dofs
 *                                [n_cells][nd]; mult [n_dofs] = cells holding the DoF; nb_off [n_cells + 1] into
 *                                nb_cell (the cells sharing a DoF with the cell, ascending, itself included) and
 *                                ov_off [pairs + 1] into (ov_i, ov_j): local indices in the cell / in the neighbour of
 *                                every shared DoF. Any output may be NULL; call with them NULL for the counts. */
int gls_vanka_sizes(gls_ctx *ctx, int *nd, int *row_floats);
int gls_vanka_element_matrices(gls_ctx *ctx, double *K);
int gls_vanka_patch_inverses(gls_ctx *ctx, double *A, float *Ainv);
int gls_vanka_sweep(gls_ctx *ctx, double *x, const double *b, double omega);
int gls_vanka_detach(gls_ctx *ctx);

/* Band-storage FP32 LU: the coarsest multigrid level's exact solve above 40000 DoFs (coarse_direct in gls_mg_params)
 * on its own, for tests and tools. An n x n matrix with lower / upper bandwidths bl / bu is kept as block columns
 * nb >= max(bl, bu, 1) wide, each one contiguous 3 nb x nb column-major panel [U_{k-1}; D_k; L_k] (3 n nb floats; no
 * n x n array in any precision), factored without pivoting by rocSOLVER / rocBLAS block calls and applied by a
 * forward / backward substitution on the panels (2 ceil(n / 128) launches, sums in a fixed order: two solves of the
 * same input are bitwise equal). There is no pivoted fallback: the factor is checked by |A x - 1| / |1| against the
 * FP64 CSR and refused (GLS_EINVAL naming the value) from 0.5 up or when not finite.
 *   gls_band_lu_layout : HOST only, no GPU. block = 0: nb = max(bl, bu) rounded up to a multiple of 256, at least
 *                        512; block > 0: nb = block, a multiple of 128 not narrower than the band. n_blocks =
 *                        ceil(n / nb), n_floats = 3 n nb (exact in 64 bits). n <= 0, a bandwidth outside 0 .. n - 1 or
 *                        a bad block: GLS_EINVAL.
 *   gls_band_lu_create : HOST CSR in FP64 (rowp of n + 1, col, val; no duplicate entries), rounded to FP32 into the
 *                        panels with row and column pin replaced by identity (pin < 0: none), factored and checked;
 *                        synchronous, on the default stream.
 *   gls_band_lu_solve  : x = A^-1 b on DEVICE vectors of n doubles (b == x allowed), x[pin] = 0; refine != 0: one
 *                        step of iterative refinement x += LU^-1 (b - A x) against the FP64 CSR. Queued on the
 *                        default stream.
 *   gls_band_lu_info   : the CSR's bandwidths, nb, the panels' bytes and the check's value; any output may be NULL. */
typedef struct gls_band_lu gls_band_lu;
int gls_band_lu_layout(int64_t n, int64_t bl, int64_t bu, int64_t block, int64_t *nb, int64_t *n_blocks, int64_t *n_floats);
int gls_band_lu_create(int64_t n, const int64_t *rowp, const int32_t *col, const double *val, int64_t pin, int64_t block,
                       gls_band_lu **handle);
int gls_band_lu_solve(gls_band_lu *handle, const double *b, double *x, int refine);
int gls_band_lu_info(const gls_band_lu *handle, int64_t *bl, int64_t *bu, int64_t *nb, int64_t *bytes, double *check);
int gls_band_lu_destroy(gls_band_lu *handle);
int gls_vanka_maps(int dim, int k, int kp, int64_t n_cells, int64_t n_vnodes, int64_t n_pnodes, const int32_t *cell_vnodes,
                   const int32_t *cell_pnodes, int32_t *cell_dofs, int32_t *mult, int64_t *nb_off, int32_t *nb_cell,
                   int64_t nb_capacity, int64_t *ov_off, uint8_t *ov_i, uint8_t *ov_j, int64_t ov_capacity,
                   int64_t *out_pairs, int64_t *out_overlaps);
/* Assembled ILU(fill) preconditioner for GMRES (replaces setup_ILU, gls_navier_stokes.cc:1161-1176:
 * Trilinos PreconditionILU(ilu_fill, ilu_atol, ilu_rtol, overlap 0) = Ifpack ILU(k), the reference's
 * 'linear solver/method = gmres' with 'ilu preconditioner fill / absolute / relative tolerance',
 * parameters.cc:546-560). The Jacobian is probed from the device operator into CSR with
 * distance-2-colored unit vectors once per Jacobian state; its graph is the reference's system
 * sparsity (constrained rows / columns hold the diagonal only, lines couple their masters). DoFs are
 * renumbered like DoFRenumbering::Cuthill_McKee; the ILU(fill) level-of-fill pattern (Ifpack_IlukGraph:
 * level(i,j) = min_k level(i,k) + level(k,j) + 1 <= fill) is inserted with explicit zeros, the
 * diagonal perturbed like Ifpack (a_ii <- rthresh a_ii + sign(a_ii) athresh) and factored by rocSPARSE
 * (multicolor order: by the color-by-color device factorization, same IKJ update order).
 * fill outside 0..GLS_ILU_MAX_FILL is rejected (GLS_EINVAL). Single rank, no multigrid. */
#define GLS_ILU_MAX_FILL 10
int gls_ilu_attach(gls_ctx *ctx, int fill, double athresh, double rthresh);
int gls_ilu_detach(gls_ctx *ctx);
/* Options of the next gls_ilu_attach.
 * ordering: GLS_ILU_ORDER_CM (default) = DoFRenumbering::Cuthill_McKee as the reference factors;
 *   GLS_ILU_ORDER_MULTICOLOR = DoFs grouped by a distance-1 coloring of the matrix's node graph
 *   (Cuthill-McKee inside a color): a different ILU (weaker, more GMRES iterations) whose triangular
 *   solves have a dependency chain of ~colors x DoFs per node instead of ~the matrix bandwidth.
 * block_dofs: block-Jacobi subdomains: the cells (in their space-filling order) are cut into
 *   ceil(n_dofs / block_dofs) contiguous ranges, couplings between the ranges are dropped and every
 *   block is factored on its own -- Ifpack's additive Schwarz with overlap 0, which is what the
 *   reference's setup_ILU gives with one block per MPI rank. 0 (default): one block. */
#define GLS_ILU_ORDER_CM 0
#define GLS_ILU_ORDER_MULTICOLOR 1
int gls_ilu_set_options(gls_ctx *ctx, int ordering, int64_t block_dofs);
int gls_ilu_info(const gls_ctx *ctx, int64_t *nnz, int *n_probes);
int gls_ilu_matrix(gls_ctx *ctx, int32_t *rowp, int32_t *col, double *val); /* probed CSR (tests) */
/* factored values in the factorization numbering (perm[dof] = row), for tests */
int gls_ilu_factors(gls_ctx *ctx, int32_t *perm, int32_t *rowp, int32_t *col, double *val);
/* Host only (no device): the ILU(fill) level-of-fill pattern of an n x n CSR graph (diagonal always
 * included, rows sorted), with each entry's level. Call with out_rowp / out_col / out_level all NULL
 * to get out_nnz; capacity = length of out_col / out_level. */
int gls_iluk_pattern(int64_t n, const int32_t *rowp, const int32_t *col, int fill, int32_t *out_rowp,
                     int32_t *out_col, int32_t *out_level, int64_t capacity, int64_t *out_nnz);
/* Host only (no device): the plan gls_ilu_attach computes on one rank from the mesh and the constraints alone.
 * Inputs as gls_create takes them (cell_pnodes NULL: the pressure sits on the velocity nodes), the constrained
 * DoFs (the Dirichlet mask's DoFs and the lines' DoFs) and the lines of gls_set_hanging without their weights;
 * fill, ordering, block_dofs as gls_ilu_attach / gls_ilu_set_options. Outputs (each may be NULL): perm[dof] = its
 * row; rowp [n_dofs + 1] / col (capacity entries) of the ILU(fill) pattern; probe[dof] = the probe vector that
 * holds the DoF's unit entry; color[dof] = its colour in the multicolor order (-1 in the Cuthill-McKee order);
 * out_nnz / out_nnz_a = entries of the ILU pattern / of the system matrix; out_n_probes; out_mc_solve = 1 when the
 * color-by-color solves apply. Call with perm, rowp, col, probe and color all NULL to get the counts. */
int gls_ilu_plan(int dim, int k, int kp, int64_t n_vnodes, int64_t n_pnodes, int64_t n_cells, const int32_t *cell_vnodes,
                 const int32_t *cell_pnodes, int64_t n_con, const int64_t *con_dofs, int64_t n_lines,
                 const int64_t *line_dofs, const int64_t *line_offsets, const int64_t *line_masters, int fill,
                 int ordering, int64_t block_dofs, int32_t *perm, int32_t *rowp, int32_t *col, int64_t capacity,
                 int32_t *probe, int32_t *color, int64_t *out_nnz, int64_t *out_nnz_a, int *out_n_probes,
                 int *out_mc_solve);
/* Host only: the DoF renumbering gls_ilu_attach uses (deal.II DoFRenumbering::Cuthill_McKee,
 * gls_navier_stokes.cc:70) on a node graph: node x's row nodes adj[adj_off[x] .. adj_off[x+1]) (itself
 * included), its DoFs dofs[dof_off[x] .. dof_off[x+1]) (old order = position in dofs);
 * order[new index] = DoF. */
int gls_cuthill_mckee(int64_t n_nodes, const int64_t *adj_off, const int64_t *adj, const int64_t *dof_off,
                      const int64_t *dofs, int64_t *order);

/* ------------------------------------------------------------------------------------------
 * Nonlinear solve: NewtonNonLinearSolver::solve (include/core/newton_non_linear_solver.h:74-139)
 * on device vectors: present (in/out, DEVICE, length n_dofs). History from gls_set_state's u1..u3
 * slots is given here explicitly.
 * ------------------------------------------------------------------------------------------ */
/* TimerOutput sections of the Newton / GMRES path (the reference's TimerOutput::Scope names,
 * gls_navier_stokes.cc:921 assemble_system, :1028 assemble_rhs, :1165 setup_ILU, :1182 setup_AMG (here
 * the geometric multigrid's setup), :1274 solve_linear_system): while enabled, gls_newton_solve
 * accumulates each section's host wall time (context stream drained at the section boundaries) and
 * call count. gls_section_timing(ctx, on) also zeroes the accumulators. */
#define GLS_SEC_ASSEMBLE_SYSTEM 0
#define GLS_SEC_ASSEMBLE_RHS 1
#define GLS_SEC_SETUP_ILU 2
#define GLS_SEC_SETUP_GMG 3
#define GLS_SEC_SOLVE_LINEAR 4
#define GLS_N_SECTIONS 5
int gls_section_timing(gls_ctx *ctx, int enable);
int gls_section_get(const gls_ctx *ctx, int section, double *seconds, int *calls);

#define GLS_NEWTON 0
#define GLS_SKIP_NEWTON 1
typedef struct {
  double tolerance;       /* non-linear solver/tolerance */
  int max_iterations;     /* non-linear solver/max iterations */
  int verbosity;          /* 0 quiet, 1 verbose (prints the reference's Newton lines) */
  gls_linear_params lin;
  int newton_iterations;  /* out */
  int linear_iterations;  /* out: total */
  int residual_evaluations; /* out */
  double final_residual;  /* out */
  int solver;             /* non-linear solver/solver: GLS_NEWTON | GLS_SKIP_NEWTON (parameters.cc:385-440) */
  int skip_iterations;    /* non-linear solver/skip iterations (skip_newton only; >= 1) */
  int is_initial_step;    /* solve_non_linear_system(method, first_iteration, force_matrix_renewal) */
  int force_matrix_renewal; /*   flags (physics_solver.h:92-96, navier_stokes_base.cc:461-590) */
  int linear_failures;    /* out: linear solves that stopped at max iterations (the reference's
                             SolverControl throws NoConvergence there; this library continues) */
} gls_newton_params;
/* Freeze (1) / release (0) the Jacobian at the current state: the skip_newton matrix reuse
 * (skip_newton_non_linear_solver.h:66-70, 126-130). While frozen, gls_jacobian_apply,
 * gls_jacobian_diagonal, the J.v linearization and the multigrid levels stay at the snapshot of
 * the state vectors and time coefficients taken here; gls_set_state / gls_set_time move only the
 * residual. gls_newton_solve with solver = GLS_SKIP_NEWTON drives this itself. */
int gls_freeze_jacobian(gls_ctx *ctx, int freeze);
int gls_newton_solve(gls_ctx *ctx, double *present, const double *u1, const double *u2, const double *u3,
                     gls_newton_params *prm);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU). Replaces the MPI domain decomposition of
 * parallel::distributed::Triangulation + Trilinos ghosted vectors (navier_stokes_base.cc:55-60,
 * gls_navier_stokes.cc:186-202) and compress(add) (:774-776).
 *   gls_part_*      : partition plan of a Morton brick mesh (host): rank-local mesh with owned
 *                     nodes first, ghosts after; import/export lists per neighbour rank.
 *   gls_dist_attach : turns a context built on the rank-local mesh into a distributed one.
 *                     Ghost import (before residual / J.v / set_state) and export-add (after)
 *                     pack into caller-owned DEVICE buffers (4 doubles per node: u,v,w,p) and call
 *                     xchg(user, 0 = import: send send_buf segments to neighbours, receive into
 *                     recv_buf | 1 = export: send recv_buf segments, receive into send_buf);
 *                     dot products sum owned DoFs and call allreduce(user, dev_buf, n) (sum).
 *                     The caller implements both with RCCL (torch.distributed "nccl") over xGMI.
 *                     Calls are made on the context stream's order; callbacks must return 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct gls_part gls_part;
int gls_part_create(int n_cells, int nodes_per_cell, const int32_t *cell_vnodes, int n_vnodes, int rank, int world,
                    gls_part **out);
int gls_part_sizes(const gls_part *p, int64_t *cell_begin, int64_t *cell_end, int64_t *n_owned_nodes,
                   int64_t *n_local_nodes, int *n_nbrs, int64_t *n_send, int64_t *n_recv);
int gls_part_get(const gls_part *p, int32_t *local_cell_vnodes, int64_t *local_to_global, int *nbr_ranks,
                 int64_t *send_offsets, int32_t *send_nodes, int64_t *recv_offsets, int32_t *recv_nodes);
int gls_part_destroy(gls_part *p);

typedef int (*gls_exchange_fn)(void *user, int phase);
typedef int (*gls_allreduce_fn)(void *user, double *dev_buf, int n);
/* red_buf: a DEVICE buffer of at least GLS_RED_BUF_MIN doubles. Every reduction the library makes
 * through the callback goes through it in pieces of at most that many values (GMRES dots: restart+1
 * <= 256, the multigrid replica's right-hand side in chunks of 256). */
#define GLS_RED_BUF_MIN 256
int gls_dist_attach(gls_ctx *ctx, int64_t n_owned_nodes, int n_nbrs, const int64_t *send_offsets,
                    const int32_t *send_nodes, const int64_t *recv_offsets, const int32_t *recv_nodes, double *send_buf,
                    double *recv_buf, double *red_buf, gls_exchange_fn xchg, gls_allreduce_fn allreduce, void *user);
/* refresh ghost entries of a DEVICE vector (e.g. the history vectors once per time step) */
int gls_dist_import(gls_ctx *ctx, double *x);
/* In-library RCCL transport (replaces the callbacks above; the reference's Trilinos ghosted vectors
 * and compress(add), gls_navier_stokes.cc:186-202, 774-776): rank 0 calls gls_rccl_unique_id and
 * broadcasts the GLS_RCCL_ID_BYTES bytes by any means; every rank calls gls_rccl_create (one
 * communicator per process, shared by all contexts, e.g. every multigrid level), then
 * gls_dist_attach_rccl per context with the gls_part_get lists. Ghost import / export-add are
 * grouped ncclSend / ncclRecv and the dot products ncclAllReduce, all on the context stream. */
#define GLS_RCCL_ID_BYTES 128
typedef struct gls_rccl gls_rccl;
int gls_rccl_unique_id(unsigned char *id_out);
int gls_rccl_create(const unsigned char *id, int rank, int world, gls_rccl **out);
int gls_rccl_destroy(gls_rccl *comm);
/* the communicator's rank and size as RCCL reports them (ncclCommUserRank / ncclCommCount) */
int gls_rccl_info(const gls_rccl *comm, int *rank, int *world);
int gls_dist_attach_rccl(gls_ctx *ctx, gls_rccl *comm, int64_t n_owned_nodes, int n_nbrs, const int *nbr_ranks,
                         const int64_t *send_offsets, const int32_t *send_nodes, const int64_t *recv_offsets,
                         const int32_t *recv_nodes);

/* General meshes across ranks (adaptive / unstructured forests; the p::d triangulation partition,
 * navier_stokes_base.cc:55-60, 682-733, ghosted vectors gls_navier_stokes.cc:186-202): any dim,
 * Qk-Qk' with separate pressure nodes, hanging-node / slip lines (DoF level, global numbering:
 * velocity node*dim + c, pressure dim*n_vnodes + node). Every rank holds the same global mesh
 * (replicated host data) and calls gls_gpart_create with its rank: contiguous equal-count ranges of
 * the given cell order per rank, node ownership by the lowest touching rank, rank-local nodes
 * owned first then ghosts (ascending (owner, id)); ghosts include the masters of the lines on local
 * cells. The rank's context is created on the local cells (gls_gpart_get) and attached with
 * gls_dist_attach_dofs (callbacks, one double per exchanged DoF) or gls_dist_attach_dofs_rccl;
 * gls_gpart_map_dofs maps global DoF ids (Dirichlet rows, line DoFs and masters) to local ones
 * (-1 where not local). Hanging lines (gls_set_hanging) are then given in local ids. */
typedef struct gls_gpart gls_gpart;
int gls_gpart_create(int dim, int k, int kp, int64_t n_cells, const int32_t *cell_vnodes, const int32_t *cell_pnodes,
                     int64_t n_vnodes, int64_t n_pnodes, int64_t n_lines, const int64_t *line_dofs,
                     const int64_t *line_offsets, const int64_t *line_masters, int rank, int world, gls_gpart **out);
int gls_gpart_sizes(const gls_gpart *p, int64_t *cell_begin, int64_t *cell_end, int64_t *n_vnodes, int64_t *n_pnodes,
                    int64_t *n_owned_vnodes, int64_t *n_owned_pnodes, int *n_nbrs, int64_t *n_send, int64_t *n_recv);
int gls_gpart_get(const gls_gpart *p, int32_t *local_cell_vnodes, int32_t *local_cell_pnodes, int64_t *vnode_l2g,
                  int64_t *pnode_l2g, int *nbr_ranks, int64_t *send_offsets, int32_t *send_dofs, int64_t *recv_offsets,
                  int32_t *recv_dofs);
int gls_gpart_map_dofs(const gls_gpart *p, int64_t n, const int64_t *global_dofs, int64_t *local_dofs);
int gls_gpart_destroy(gls_gpart *p);
/* The same plan from the rank's LOCAL PART only (distributed forest: no rank holds the global mesh;
 * the p::d triangulation's locally relevant cells, navier_stokes_base.cc:55-60): the owned cells
 * (cell_owner == rank, in the given order) plus the ghost layer -- every cell sharing a node with an
 * owned cell, and every cell touching a MASTER node of a hanging line whose DoF lies on an owned cell
 * (e.g. the far corner / edge midpoints of a coarse face) -- each with its owner; the lines whose DoF
 * lies on a provided cell. A node is owned by the lowest rank among ALL cells touching it, so each node
 * the rank needs must come with every cell touching it: with a thinner layer (p4est's one-cell ghost
 * layer alone) two ranks can disagree on an owner and on the exchange lists. A needed master node that
 * lies on no provided cell is rejected (GLS_EINVAL); a missing cell of a provided node cannot be seen
 * locally -- dist.local_part() builds the layer by this rule. Nodes are 64-bit keys unique over
 * the forest (no global numbering needed); DoF keys are key * (dim + 1) + c with c = dim for pressure
 * (line_dofs / line_masters and gls_gpart_map_dofs use DoF keys). cell_pkeys = NULL for equal order.
 * vnode_l2g / pnode_l2g of gls_gpart_get return the local nodes' keys; the exchange lists are those of
 * gls_gpart_create for the same partition (identical arrays when the keys are the global node ids).
 * A global numbering, if wanted, is one exclusive scan of the owned counts plus one exchange. */
int gls_dpart_create(int dim, int k, int kp, int64_t n_cells, const int32_t *cell_owner, const int64_t *cell_vkeys,
                     const int64_t *cell_pkeys, int64_t n_lines, const int64_t *line_dofs, const int64_t *line_offsets,
                     const int64_t *line_masters, int rank, int world, gls_gpart **out);
int gls_dist_attach_dofs(gls_ctx *ctx, int64_t n_owned_vnodes, int64_t n_owned_pnodes, int n_nbrs,
                         const int64_t *send_offsets, const int32_t *send_dofs, const int64_t *recv_offsets,
                         const int32_t *recv_dofs, double *send_buf, double *recv_buf, double *red_buf,
                         gls_exchange_fn xchg, gls_allreduce_fn allreduce, void *user);
int gls_dist_attach_dofs_rccl(gls_ctx *ctx, gls_rccl *comm, int64_t n_owned_vnodes, int64_t n_owned_pnodes,
                              int n_nbrs, const int *nbr_ranks, const int64_t *send_offsets, const int32_t *send_dofs,
                              const int64_t *recv_offsets, const int32_t *recv_dofs);

/* ------------------------------------------------------------------------------------------
 * Host-side building blocks (host pointers).
 * ------------------------------------------------------------------------------------------ */
/* bdf_coefficients (source/core/bdf.cc:45-75): alpha[order+1] */
int gls_bdf_coefficients(int order, const double *dt, int n_dt, double *alpha);
/* sdirk_coefficients (source/core/sdirk.cc:11-44): out[order*(order+1)] row-major */
int gls_sdirk_coefficients(int order, double dt, double *out);
/* Transient simulation control: SimulationControlTransient (source/core/simulation_control.cc:84-147) and,
 * with output_control = GLS_OUTPUT_TIME, SimulationControlTransientDynamicOutput (:173-218). Parameters
 * are the 'simulation control' entries 'time step', 'time end', 'adapt', 'max cfl', 'adaptative time step
 * scaling', 'output control', 'output frequency', 'output time' (parameters.cc:27-71, 109-131).
 *   gls_time_control_integrate: integrate() (:109-122) -- returns 0 at the end (time >= time_end -
 *     1e-12 * step, :126-130), else increments the iteration, takes the next step, shifts the four stored
 *     steps (newest first, add_time_step :28-38) and advances the time; returns 1.
 *   The next step, calculate_time_step (:132-147): the present step; with adapt from iteration 2 on
 *     step * scaling, or step * max_cfl / CFL when CFL > 0 and max_cfl / CFL < scaling; then clamped to
 *     land on time_end. GLS_OUTPUT_TIME (:180-206; the reference's class scales the step whatever 'adapt'
 *     says, and so does this one): the step is also clamped to land on the next multiple of output_time
 *     (a forced output step), and the step after a forced one is the step before it (steps[1]) again.
 *   gls_time_control_set_cfl: set_CFL, the CFL of the iteration just solved (gls_flow_diagnostics' out[0]).
 *   gls_time_control_is_output_iteration: GLS_OUTPUT_ITERATION iteration % output_frequency == 0 (:40-44);
 *     GLS_OUTPUT_TIME (:208-218) time - last output time > output_time (1 - 1e-12), and the last output
 *     time then becomes the present time: a side effect, as in the reference -- call it once per iteration.
 *   gls_time_control_get: iteration, time, step, the four stored steps (any pointer may be NULL).
 * With adapt off and GLS_OUTPUT_ITERATION the step is constant but for the final clamp. Host only. */
#define GLS_OUTPUT_ITERATION 0
#define GLS_OUTPUT_TIME 1
typedef struct {
  double dt, time_end;
  int adapt;
  double max_cfl, scaling;
  int output_control;     /* GLS_OUTPUT_ITERATION | GLS_OUTPUT_TIME */
  int output_frequency;   /* GLS_OUTPUT_ITERATION: >= 1 */
  double output_time;     /* GLS_OUTPUT_TIME: > 0 */
} gls_time_control_params;
typedef struct gls_time_control gls_time_control;
int gls_time_control_create(const gls_time_control_params *prm, gls_time_control **out);
void gls_time_control_destroy(gls_time_control *tc);
int gls_time_control_integrate(gls_time_control *tc);
int gls_time_control_set_cfl(gls_time_control *tc, double cfl);
int gls_time_control_get(const gls_time_control *tc, int *iteration, double *time, double *time_step, double steps[4]);
int gls_time_control_is_output_iteration(gls_time_control *tc);
/* Newton driver KAT: the reference's fake physics x0^2+x1=0, 2x1+3=0
 * (tests/core/non_linear_test_system_01.h:50-129) through the same Newton template. */
int gls_newton_selftest(double x_out[2]);
/* SkipNewton KAT (tests/core/skip_newton_non_linear_solver_01.cc): same fake physics through the
 * SkipNewton template (skip_newton_non_linear_solver.h:54-131), tol 1e-8, 10 iterations. */
int gls_skip_newton_selftest(int skip_iterations, double x_out[2]);

/* hyper_cube mesh + canonical DoF numbering (GridGenerator::hyper_cube + refine_global,
 * source/core/grids.cc:12-60). Periodic directions identify the high face with the low face.
 * Cells are emitted in Morton (p4est z-)order. Arrays are allocated by the caller with the
 * sizes from gls_mesh_hyper_cube_sizes. boundary ids: colorize ? 2d / 2d+1 : 0. */
int gls_mesh_hyper_cube_sizes(int dim, int n, int k, int kp, int periodic_mask,
                              int64_t *n_cells, int64_t *n_vnodes, int64_t *n_pnodes);
int gls_mesh_hyper_cube(int dim, int n, int k, int kp, double lo, double hi, int periodic_mask,
                        int32_t *cell_vnodes, int32_t *cell_pnodes, double *cell_x0, double *cell_h);

/* subdivided_hyper_rectangle mesh (GridGenerator::subdivided_hyper_rectangle + refine_global): cells[a] cells on axis
 * a of the box p1 .. p2, each count even and >= 2; dim = 3 only (GLS_EINVAL otherwise). The same arrays as
 * gls_mesh_hyper_cube, cell_h[c] = (p2 - p1) / cells per axis. Nodes: the lexicographic lattice, x fastest, with
 * K cells[a] + 1 nodes on axis a, K cells[a] where bit a of periodic_mask is set (the high face is the low face).
 * Cells: bricks of 2 x 2 x 2 cells, a brick's 8 cells in the order cx + 2 cy + 4 cz, the bricks in "tile-Morton"
 * order: nb[a] = cells[a] / 2 bricks per axis, s = the largest power of two dividing all three nb[a]; tiles of s^3
 * bricks run lexicographically, tx fastest, and the bricks of a tile in Morton order of (bx % s, by % s, bz % s):
 *   brick(bx, by, bz) = ((tz nty + ty) ntx + tx) s^3 + morton3(bx % s, by % s, bz % s),  t = b / s, nt = nb / s.
 * cells = (n, n, n) with n a power of two is the Morton order: the arrays equal gls_mesh_hyper_cube's bit for bit.
 * A context created on the open mesh (mask 0, nb[a] <= 2048) recognises the lattice and sums the brick-surface slab
 * by this closed form instead of the index map (GLS_SLAB_CSR=1 at gls_create: the map). boundary ids: the cube's,
 * colorize ? 2d / 2d+1 : 0. */
int gls_mesh_hyper_rectangle_sizes(int dim, const int cells[3], int k, int kp, int periodic_mask,
                                   int64_t *n_cells, int64_t *n_vnodes, int64_t *n_pnodes);
int gls_mesh_hyper_rectangle(int dim, const int cells[3], int k, int kp, const double p1[3], const double p2[3],
                             int periodic_mask, int32_t *cell_vnodes, int32_t *cell_pnodes, double *cell_x0,
                             double *cell_h);

/* Locally refined hyper_cube (one extra level): hyper_cube(lo, hi) with n^dim cells, the cells
 * flagged in refine[n^dim] (lexicographic, x fastest; NULL = none) split into 2^dim children
 * (execute_coarsening_and_refinement on a p4est forest, navier_stokes_base.cc:592-780). Nodes are
 * numbered lexicographically on the fine node lattice; hanging nodes are constrained to the
 * unrefined neighbour's nodes: value(node) = sum_j w_j value(master_j) (node level, for every
 * component; see gls_set_hanging for the DoF-level lines). Velocity FE_Q(k) and pressure
 * FE_Q(kp) spaces, 1 <= kp <= k <= 2. Owned storage, freed by gls_mesh_refined_destroy. */
typedef struct {
  int dim, k, kp;
  int64_t n_cells, n_vnodes, n_pnodes;
  const int32_t *cell_vnodes;   /* [n_cells][(k+1)^dim] lexicographic local order */
  const int32_t *cell_pnodes;   /* [n_cells][(kp+1)^dim] */
  const int32_t *cell_level;    /* [n_cells] 0 unrefined, 1 child of a refined cell */
  const double *cell_x0, *cell_h;  /* [n_cells][dim] */
  const double *vnode_x, *pnode_x; /* [n_vnodes][dim], [n_pnodes][dim] */
  int64_t n_vhang;              /* hanging velocity node vhang_node[i] = sum over j in           */
  const int64_t *vhang_node;    /*   [vhang_off[i], vhang_off[i+1]) of vhang_w[j] * node          */
  const int64_t *vhang_off;     /*   vhang_master[j]                                              */
  const int64_t *vhang_master;
  const double *vhang_w;
  int64_t n_phang;              /* the same for the pressure nodes */
  const int64_t *phang_node, *phang_off, *phang_master;
  const double *phang_w;
  void *impl_;                  /* owned storage (opaque) */
} gls_refined_mesh;
int gls_mesh_refined_create(int dim, int n, int k, int kp, double lo, double hi, const int32_t *refine,
                            gls_refined_mesh **out);
int gls_mesh_refined_destroy(gls_refined_mesh *mesh);
/* Multi-level adaptive refinement of a hyper_cube (the reference's p4est forest,
 * navier_stokes_base.cc:55-60, 592-780): an octree over n^dim level-0 cells, leaves in p4est's
 * depth-first Morton order. gls_octree_adapt refines flagged leaves (below max_level), coarsens
 * complete sibling groups that are all flagged (above min_level) when that keeps the vertex 2:1
 * balance, and restores the balance by refinement (limit_level_difference_at_vertices).
 * gls_octree_mesh builds the FE_Q(k) x FE_Q(kp) node spaces with hanging lines whose masters are
 * all unconstrained (make_hanging_node_constraints + close()), as a gls_refined_mesh (free it with
 * gls_octree_mesh_destroy); gls_octree_transfer is SolutionTransfer between two such meshes of the
 * same cube (host vectors, [velocity node-major | pressure]). */
typedef struct gls_octree gls_octree;
int gls_octree_create(int dim, int n, gls_octree **out);
void gls_octree_destroy(gls_octree *tree);
/* Periodic directions (bit d of mask; before adapting): the balance, the smoothing's neighbourhoods and
 * the Kelly faces wrap around them, and gls_octree_mesh identifies the max face's nodes with the min
 * face's, hanging lines included (periodicity under local refinement, gls_navier_stokes.cc:130-134,
 * 164-168: make_periodicity_constraints closed together with the hanging-node constraints). */
int gls_octree_set_periodic(gls_octree *tree, int mask);
int gls_octree_info(const gls_octree *tree, int64_t *n_cells, int *max_level);
int gls_octree_cells(const gls_octree *tree, int32_t *level, double *x0, double *h, double lo, double hi);
int gls_octree_adapt(gls_octree *tree, const int32_t *refine, const int32_t *coarsen, int max_level, int min_level);
/* Triangulation::prepare_coarsening_and_refinement with the reference's mesh smoothing
 * (smoothing_on_refinement | smoothing_on_coarsening, navier_stokes_base.cc:55-60, called at :682):
 * do_not_produce_unrefined_islands, eliminate_refined_inner/boundary_islands,
 * limit_level_difference_at_vertices, eliminate_unrefined_islands, no double refinement at faces,
 * complete-family coarsening that keeps the 2:1 rule (fix_coarsen_flags), iterated until the flags no
 * longer change. refine / coarsen: per-leaf flags in the tree's order, updated in place. Returns the
 * number of iterations. */
int gls_octree_prepare(const gls_octree *tree, int32_t *refine, int32_t *coarsen);
int gls_octree_mesh(const gls_octree *tree, int k, int kp, double lo, double hi, gls_refined_mesh **out);
int gls_octree_mesh_destroy(gls_refined_mesh *mesh);
int gls_octree_transfer(const gls_refined_mesh *old_mesh, const gls_refined_mesh *new_mesh, const double *old_vec,
                        double *new_vec);
/* Kelly error indicator per cell: KellyErrorEstimator<dim>::estimate as
 * refine_mesh_kelly calls it (navier_stokes_base.cc:612-652) — face rule QGauss<dim-1>(n_q + 1),
 * no Neumann boundaries (boundary faces add nothing), deal.II's default cell_diameter_over_24:
 * eta_K = sqrt(sum over interior faces F of K of diam(K)/24 * int_F sum_c [d u_c / dn]^2) over the
 * velocity components (variable 0) or the pressure (variable 1). Conforming meshes (no hanging
 * nodes). sol, eta: DEVICE pointers (eta: n_cells doubles; deal.II stores them as float). */
int gls_kelly_estimate(gls_ctx *ctx, const double *sol, int variable, double *eta);
/* The same on meshes with hanging faces (gls_octree_mesh): the face pieces from gls_octree_faces
 * (the fine side of a non-conforming face is one piece; deal.II integrates over the subfaces), the
 * integrals on the device, each piece counted for both of its cells. sol, eta: DEVICE pointers. */
int gls_kelly_estimate_faces(gls_ctx *ctx, const double *sol, int variable, int64_t n_faces, const int32_t *fa,
                             const int32_t *fb, const int32_t *fdir, const double *rect_a, const double *rect_b,
                             double *eta);
int gls_octree_faces(const gls_refined_mesh *mesh, int64_t *n_faces, int32_t *fa, int32_t *fb, int32_t *fdir,
                     double *rect_a, double *rect_b);
/* Level meshes of a geometric multigrid on the refinement hierarchy (global coarsening; the reference's
 * level hierarchy of the p4est forest, not a reference interface -- its GLS solver uses ILU / ML-AMG,
 * gls_navier_stokes.cc:1161-1240): a copy of the forest with every leaf finer than `level` replaced by
 * its ancestor on `level` (2:1 balance preserved). Free with gls_octree_destroy. */
int gls_octree_coarsen_to(const gls_octree *tree, int level, gls_octree **out);
/* Prolongation between two nested octree meshes (coarse = a coarsening of fine): DoF-level CSR over the
 * fine DoFs, fine DoF i = sum_j P_ij coarse DoF j = the conforming coarse field (hanging nodes from their
 * lines) interpolated at the fine node; rows of fine hanging DoFs are empty, columns are coarse masters.
 * off: n_dofs(fine)+1, col / w: nnz; inject: n_dofs(coarse), the fine DoF at each coarse DoF's position.
 * off == NULL: nnz only. Host arrays; non-periodic. */
int gls_octree_mg_transfer(const gls_refined_mesh *fine, const gls_refined_mesh *coarse, int64_t *nnz, int64_t *off,
                           int32_t *col, double *w, int64_t *inject);
/* The same on mapped (MappingQ) meshes, conforming or adapted: pieces and geometry from
 * gls_fe_space_kelly_faces with nq = n_q + 1 (nqf = nq^(dim-1) points per piece, host arrays),
 * the jump integrals on the device; eta (DEVICE, n_cells) = sqrt(cell_diam/24 * sum of pieces). */
int gls_kelly_estimate_mapped(gls_ctx *ctx, const double *sol, int variable, int64_t n_pieces, int nqf,
                              const int32_t *ca, const int32_t *cb, const double *xi, const double *g,
                              const double *jxw, const double *cell_diam, double *eta);
/* Forces and torques on the boundaries: the reference's calculate_forces / calculate_torques
 * (postprocessing_force.cc:67-110, postprocessing_torque.cc:67-125; called after every solved iteration,
 * navier_stokes_base.cc:120-250, 855-881). Over the boundary faces, with QGauss<dim-1>(k + 1) and the
 * cells' MappingQ: n = -(outward unit normal), sigma = nu (grad u + grad u^T) - p I,
 *   f += sigma n JxW,   T += (x_q - cor) x (sigma n JxW)   (2D: T_z only; T always has 3 components).
 * gls_boundary_plan_create uploads the face data of one mesh (host arrays: gls_fe_space_boundary_faces'
 * layout -- per face its cell and its slot = row of the tables, slot -1 = skipped; per point xi / normal
 * / xq [f][q][dim], jinv [f][q][dim][dim], jxw [f][q]; box meshes pass a diagonal jinv); rebuild it after
 * an adaptation. gls_boundary_loads evaluates a solution vector on the DEVICE (the context's layout) in
 * one pass over all boundaries (the reference makes one pass per boundary) and returns
 * force[n_slots][3] / torque[n_slots][3] to HOST arrays; cor[n_slots][3] (host) is the centre of rotation
 * of each slot. The sums use no atomics and a fixed order: two calls give bitwise identical tables.
 * Kernels exist for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}; other degrees (2D Q3) are GLS_EINVAL. */
typedef struct gls_boundary_plan gls_boundary_plan;
int gls_boundary_plan_create(gls_ctx *ctx, int64_t n_faces, int nqf, const int32_t *cell, const int32_t *slot,
                             const double *xi, const double *jinv, const double *normal, const double *jxw,
                             const double *xq, int n_slots, gls_boundary_plan **plan);
int gls_boundary_plan_destroy(gls_boundary_plan *plan);
int gls_boundary_loads(gls_ctx *ctx, gls_boundary_plan *plan, const double *sol, double viscosity, const double *cor,
                       double *force, double *torque);
/* Flow diagnostics of a solution vector in one pass over the context's cells, on the DEVICE (sol: the
 * context's layout, constrained DoFs holding their values as after gls_apply_dirichlet):
 *   out[0] = max over cells of |u(centre)| dt / h: calculate_CFL (postprocessing_cfl.cc:36-87) -- the velocity
 *            at the reference cell's centre, h = sqrt(4|K|/pi)/deg (2D), (6|K|/pi)^(1/3)/deg (3D), deg =
 *            max(k, kp), |K| = cell->measure() (box cells: the product of cell_h; mapped cells: from the
 *            corner support points);
 *   out[1] = int 1/2 |u|^2, out[2] = int 1/2 |curl u|^2 (2D: omega_z only), out[3] = sum of JxW, with the
 *            context's QGauss(k+1) and its JxW / J^-1 per quadrature point (calculate_kinetic_energy,
 *            postprocessing_kinetic_energy.cc, and calculate_enstrophy, postprocessing_enstrophy.cc, divide
 *            out[1], out[2] by the volume).
 * Every layout of a context: brick, per-cell box, mapped, with hanging lines; a distributed context sums its
 * own cells (ghost values of sol must be current: gls_dist_import), the caller combines the ranks.
 * Per-block partials, then one ordered stage on the device: no atomics, two calls on the same input are
 * bitwise equal. The work is queued on the context's stream; the buffers are allocated at the first call;
 * out (HOST) is one download of 4 doubles. Kernels exist for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}
 * with QGauss(k+1); other degrees (2D Q3) are GLS_EINVAL. */
int gls_flow_diagnostics(gls_ctx *ctx, const double *sol, double dt, double out[4]);
/* The point data of a VTU piece evaluated on the DEVICE: what gls_vtu_write (below) derives on the host from a
 * host vector, from a device vector (the context's layout, constrained DoFs holding their values) in one launch
 * over all cells: for every cell and every patch point of DataOut::build_patches(mapping, subdivision)
 * (navier_stokes_base.cc:1035-1064, post_processors.h:27-171), point P = cell * npp + p with p x-fastest over
 * the (subdivision+1)^dim lattice,
 *   points [P][3], velocity [P][3] (2D: z = 0), pressure [P], vorticity [P][3] (3D) or [P] (2D),
 *   q_criterion [P] = 0.5 (sum_{p' <= p} |W|^2 - sum_{p' <= p} |S|^2) over the cell's points in patch order (the
 *   reference's accumulators live outside its point loop, post_processors.h:84-115; the sums restart at every
 *   cell), velocity_eulerian [P][3] = u + omega x x when the mesh has srf.
 * gls_output_plan_create uploads the geometry the patch points need (box cells: cell_x0 / cell_h; mapped cells:
 * cell_support, (map_degree+1)^dim dim doubles per cell) and the 1D tables at t / subdivision, and allocates the
 * device field buffers once. mesh must be the description the context was created from (dim, k, kp, n_cells and
 * map_degree are checked; srf / omega are the mesh's); rebuild the plan after an adaptation. Every layout of a
 * context: brick, per-cell box, mapped, with hanging lines. gls_output_fields: the launch, then one download per
 * array into HOST arrays (velocity_eulerian may be NULL without srf). gls_vtu_write_device: the same, then the
 * file writer of gls_vtu_write -- equal arrays give equal bytes; the connectivity and subdomain arrays are
 * gls_vtu_write's. The work is queued on the context's stream; no atomics, two calls on the same input are
 * bitwise equal. With GLS_OUTPUT_SPLIT set in the environment gls_vtu_write_device prints its host seconds (launch
 * and downloads, base64 encoding, the rest of the writer) on stderr. Kernels exist for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}, box and mapped (map_degree <= 3), with (subdivision+1)^dim <= 256
 * (subdivision 1..15 in 2D, 1..5 in 3D); anything else (2D Q3) is GLS_EINVAL at gls_output_plan_create. */
typedef struct gls_output_plan gls_output_plan;
int gls_output_plan_create(gls_ctx *ctx, const gls_mesh_desc *mesh, int subdivision, gls_output_plan **plan);
int gls_output_plan_destroy(gls_output_plan *plan);
int gls_output_fields(gls_ctx *ctx, gls_output_plan *plan, const double *sol, double *points, double *velocity,
                      double *pressure, double *vorticity, double *q_criterion, double *velocity_eulerian);
int gls_vtu_write_device(gls_ctx *ctx, gls_output_plan *plan, const double *sol, const char *filename, int subdomain,
                         int binary);
/* GridRefinement::refine_and_coarsen_fixed_number, refinement part (navier_stokes_base.cc:654-661;
 * serial deal.II rule): flags[i] = 1 for the int(top_fraction * n_cells) largest criteria (every
 * cell >= the threshold value). Returns the number of flagged cells. HOST arrays. */
int gls_refine_fixed_number(int64_t n_cells, const float *criteria, double top_fraction, int32_t *flags);
/* parallel::distributed::GridRefinement::refine_and_coarsen_fixed_number (fraction_type 0) and
 * refine_and_coarsen_fixed_fraction (fraction_type 1), refinement part — the calls refine_mesh_kelly
 * makes (navier_stokes_base.cc:654-667; deal.II 9.2 distributed/grid_refinement.cc): bisection for
 * the threshold (25 steps at most) between the widened extremes of the criteria, the target being
 * int(f * n_cells) cells (f = top_fraction capped by adjust_refine_and_coarsen_number_fraction<dim>
 * so the refined mesh has at most max_n_cells cells) or top_fraction of the summed criteria;
 * flags[i] = 1 where criteria[i] >= threshold. criteria >= 0 over ALL cells (gathered), HOST
 * arrays; threshold may be NULL. Returns the number of flagged cells. */
int gls_refine_pd(int64_t n_cells, const float *criteria, int dim, int fraction_type, double top_fraction,
                  int64_t max_n_cells, int32_t *flags, double *threshold);
/* The same with coarsening (fraction coarsening = bottom_fraction): adjust_refine_and_coarsen_
 * number_fraction<dim> caps both fractions (and coarsens (n - max) / (1 - 2^-dim) cells when the mesh
 * already has max_n_cells); the bottom threshold leaves int((1 - bottom) * n) cells (or that fraction
 * of the summed criteria) above it, the lowest float when bottom = 0; mark_cells: refine[i] = 1 where
 * criteria >= top (GridRefinement::refine), coarsen[i] = 1 where criteria <= bottom and not refine
 * (GridRefinement::coarsen). thresholds[2] = {top, bottom} (may be NULL). Returns the refined count. */
int gls_refine_coarsen_pd(int64_t n_cells, const float *criteria, int dim, int fraction_type, double top_fraction,
                          double bottom_fraction, int64_t max_n_cells, int32_t *refine, int32_t *coarsen,
                          double *thresholds);
/* SolutionTransfer::interpolate (navier_stokes_base.cc:689-733) for the first refinement of the
 * uniform hyper_cube(n, lo, hi) that `mesh` was built from: coarse in canonical lattice numbering
 * ([velocity node-major | pressure]), fine in the refined mesh's numbering. HOST arrays. */
int gls_mesh_refined_interpolate(const gls_refined_mesh *mesh, int n, double lo, double hi, const double *coarse,
                                 double *fine);

/* ------------------------------------------------------------------------------------------
 * Unstructured quadrilateral / hexahedral meshes, host side.
 * gls_umesh_generate: GridGenerator::generate_from_name_and_arguments (source/core/grids.cc:30-36)
 *   for hyper_cube ("lo : hi : colorize"), hyper_rectangle ("p1 : p2 : colorize"),
 *   subdivided_hyper_rectangle ("n1,n2[,n3] : p1 : p2 : colorize"), hyper_shell (2D,
 *   "center : inner : outer : n_cells : colorize"; inner boundary 0, outer 1; SphericalManifold on
 *   every object), cylinder (3D, "radius : half_length"; axis x, hull 0, x = -L 1, x = +L 2;
 *   CylindricalManifold on the hull) and cylinder_shell (3D, "length : inner : outer : n_radial :
 *   n_axial"; axis z, builder-defined colouring inner 0, outer 1, z = 0 2, z = length 3;
 *   CylindricalManifold on every object).
 * gls_umesh_read_gmsh: GridIn::read_msh (grids.cc:21-28), ASCII 2.2 / 4.0 / 4.1; quads (2D) or
 *   hexes (3D); boundary id = physical tag of the boundary element (the entity tag when none).
 * gls_umesh_set_manifold / gls_umesh_boundary_manifold: set_manifold + set_all_manifold_ids_on_
 *   boundary (source/core/manifolds.cc:226-247); type 0 flat, 1 spherical(center), 2 cylindrical
 *   (axis through center).
 * gls_umesh_refine_global: refine_global with deal.II 9.2's new-vertex placement (line midpoints
 *   on the line's manifold, quad / hex centres by transfinite-interpolation weights); cells stay
 *   parent-major (children of cell c are 2^dim c + lexicographic child index).
 * gls_umesh_fe_space: FE_Q(k)^dim x FE_Q(kp) nodes (1 <= kp <= k <= 2), MappingQ(k, qmapping_all)
 *   support points per cell, node support points, boundary-id bits per node (bit b: the node lies
 *   on a boundary face with id b), cell->measure(); periodic pairs (id_a, id_b, direction) triples
 *   identify the nodes of id_b with their translates on id_a (make_periodicity_constraints).
 * gls_fe_space_transfer: SolutionTransfer::interpolate across one global refinement (HOST vectors).
 * ------------------------------------------------------------------------------------------ */
typedef struct gls_umesh gls_umesh;
typedef struct {
  int dim, k, kp;
  int64_t n_cells, n_vnodes, n_pnodes;
  const int32_t *cell_vnodes, *cell_pnodes;   /* [n_cells][(k+1)^dim], [n_cells][(kp+1)^dim] lexicographic */
  const double *vnode_x, *pnode_x;            /* [n][dim] support points (mapped) */
  const uint32_t *vnode_bid, *pnode_bid;      /* boundary-id bits per node */
  const double *cell_support;                 /* [n_cells][(k+1)^dim][dim]: gls_mesh_desc.cell_support, map_degree = k */
  const int32_t *cell_mapping;                /* mapping degree used per cell (1 or k) */
  const double *cell_measure;                 /* cell->measure() */
  double volume;                              /* GridTools::volume (sum of measures) */
  const int32_t *cell_level;                  /* refinement level of each active cell */
  int64_t n_vhang;                            /* hanging velocity node vhang_node[i] = sum over j in    */
  const int64_t *vhang_node, *vhang_off;      /*   [vhang_off[i], vhang_off[i+1]) of vhang_w[j] * node   */
  const int64_t *vhang_master;                /*   vhang_master[j] (make_hanging_node_constraints +      */
  const double *vhang_w;                      /*   close(); masters unconstrained)                       */
  int64_t n_phang;                            /* the same for the pressure nodes */
  const int64_t *phang_node, *phang_off, *phang_master;
  const double *phang_w;
  void *impl_;
} gls_fe_space;
int gls_umesh_generate(int dim, const char *grid_type, const char *grid_arguments, gls_umesh **out);
int gls_umesh_read_gmsh(int dim, const char *path, gls_umesh **out);
int gls_umesh_set_manifold(gls_umesh *mesh, int manifold_id, int type, const double *center, const double *axis);
int gls_umesh_boundary_manifold(gls_umesh *mesh, int boundary_id, int manifold_id);
int gls_umesh_refine_global(gls_umesh *mesh, int times);
int gls_umesh_info(const gls_umesh *mesh, int64_t *n_cells, int64_t *n_vertices, double *volume);
void gls_umesh_destroy(gls_umesh *mesh);
int gls_umesh_fe_space(const gls_umesh *mesh, int k, int kp, int qmapping_all, int n_periodic,
                       const int32_t *periodic, gls_fe_space **out);
int gls_fe_space_destroy(gls_fe_space *space);
int gls_fe_space_transfer(const gls_fe_space *coarse, const gls_fe_space *fine, const double *coarse_vec,
                          double *fine_vec);
/* Local adaptation of the triangulation (the reference's p::d::Triangulation with
 * smoothing_on_refinement | smoothing_on_coarsening, navier_stokes_base.cc:55-60, 592-780), on any
 * mesh above (gmsh, generators, manifolds; new vertices placed as refine_global places them):
 *   gls_umesh_prepare: prepare_coarsening_and_refinement with that smoothing (the steps of
 *     gls_octree_prepare, neighbours through shared faces); refine / coarsen are per-active-cell
 *     flags in the order of gls_umesh_fe_space's cells, updated in place; returns the iterations.
 *   gls_umesh_adapt: execute_coarsening_and_refinement: flagged cells refined, complete flagged
 *     families coarsened when the vertex 2:1 balance allows, balance restored by refinement.
 * A space built afterwards carries the hanging-node lines (gls_fe_space.vhang_* / phang_*) and its
 * cells' levels; gls_fe_space_transfer then maps vectors from any earlier space of the same mesh
 * (refinement, coarsening, several levels). */
int gls_umesh_prepare(const gls_umesh *mesh, int32_t *refine, int32_t *coarsen);
/* Unit normals at the velocity nodes of the boundary faces with id boundary_id (the averaged face
 * normals VectorTools::compute_no_normal_flux_constraints uses for a slip boundary,
 * gls_navier_stokes.cc:100-110); [n_vnodes][dim], zero off that boundary. Host array. */
int gls_fe_space_boundary_normals(const gls_fe_space *space, int boundary_id, double *normals);
/* Edges and corners of a slip boundary (compute_no_normal_flux_constraints constrains as many
 * velocity components as independent normal directions meet at a node): the node's face normals
 * grouped by direction (groups within 60 degrees merge: a smooth curved wall gives one), count[v] =
 * the rank of the group means (0 off the boundary, 1, 2 = an edge in 3D, dim = all components);
 * normals: [n_vnodes][3][dim], row i = unit mean of group i (row 0 = the node normal when count = 1). */
int gls_fe_space_boundary_normal_sets(const gls_fe_space *space, int boundary_id, int32_t *count, double *normals);
int gls_umesh_adapt(gls_umesh *mesh, const int32_t *refine, const int32_t *coarsen);
/* Periodic boundary pairs of the triangulation (the reference's add_periodicity after
 * collect_periodic_faces, grids.cc:41-58): n_periodic triples (id a, id b, direction). gls_umesh_prepare
 * then treats the faces across them as neighbours (mesh smoothing) and gls_umesh_adapt / the vertex 2:1
 * balance identify the translated vertices, so refinement levels differ by at most one across a periodic
 * boundary. A space built with the same pairs (gls_umesh_fe_space) identifies the partnered nodes and
 * constrains the nodes of a finer face to the coarser face across the boundary
 * (make_periodicity_constraints, gls_navier_stokes.cc:128-134, 162-168), and its Kelly faces
 * (gls_fe_space_kelly_faces) include the periodic face pieces. */
int gls_umesh_set_periodic(gls_umesh *mesh, int n_periodic, const int32_t *periodic);
/* Level meshes of a geometric multigrid on the triangulation's refinement hierarchy (global coarsening):
 * a copy whose active cells are the current ones with every cell finer than `level` replaced by its
 * ancestor on `level` (free with gls_umesh_destroy). gls_fe_space_mg_transfer: the prolongation between
 * the FE spaces of two such levels (coarse = a coarsening of fine's triangulation) as a DoF-level CSR over
 * the fine DoFs -- FE_Q's embedding of the coarse cell's field (hanging nodes from their lines) at the fine
 * node's reference position, whatever the mapping; fine hanging rows empty, coarse masters as columns --
 * and inject (n_dofs(coarse)): the fine DoF at each coarse DoF's node. off == NULL: nnz only. Feed both to
 * gls_mg_attach_transfers (the reference preconditions these meshes with ILU / ML-AMG,
 * gls_navier_stokes.cc:1161-1240). A P-LEVEL PAIR -- the same active cells (two spaces of one triangulation, or
 * of copies with the same hierarchy), the coarse space of lower degree (Q2-Q1 -> Q1-Q1) -- gives the coarse
 * degree's interpolant at the fine nodes (FE_Q's embedding of the lower degree) and the injection at the
 * shared nodes (the fine degree a multiple of the coarse one); other degree mismatches are GLS_EINVAL. */
int gls_umesh_coarsen_to(const gls_umesh *mesh, int level, gls_umesh **out);
int gls_fe_space_mg_transfer(const gls_fe_space *fine, const gls_fe_space *coarse, int64_t *nnz, int64_t *off,
                             int32_t *col, double *w, int64_t *inject);
/* Face pieces for KellyErrorEstimator with MappingQ on such a space (conforming faces one piece,
 * a face with a refined neighbour one piece per child face; geometry on the coarse side as deal.II's
 * present cell): cells ca / cb, and per QGauss<dim-1>(nq) point q of piece e the reference
 * coordinates xi[e][q][side][dim] of both sides, g[e][q][side][dim] = J^-1 n, jxw[e][q];
 * cell_diam[n_cells] = cell->diameter(). Host arrays; call with ca == NULL for the count. */
int gls_fe_space_kelly_faces(const gls_fe_space *space, int nq, int64_t *n_pieces, int32_t *ca, int32_t *cb,
                             double *xi, double *g, double *jxw, double *cell_diam);
/* Boundary faces of the active cells, for the reference's force / torque post-processing
 * (postprocessing_force.cc, postprocessing_torque.cc): per face its cell, local face 2*d + side and
 * boundary id; per point q of QGauss<dim-1>(nq) (nqf = nq^(dim-1), first tangential direction fastest)
 * the reference coordinates xi[f][q][dim], the inverse Jacobian jinv[f][q][a][i] = d xi_a / d x_i
 * (grad u = J^-T grad_xi u), the OUTWARD unit normal[f][q][dim], jxw[f][q] and the mapped point
 * xq[f][q][dim], with the MappingQ geometry of the Kelly pieces (the cell's cell_mapping degree). Every
 * face with at_boundary() is listed, on adapted meshes once per active cell. The faces of a periodic
 * pair are NOT taken out: they are boundary faces of the triangulation and the reference would integrate
 * over them for a bc of type periodic with that id, so they are listed with their id. Host arrays;
 * call with all arrays NULL for the count. */
int gls_fe_space_boundary_faces(const gls_fe_space *space, int nq, int64_t *n_faces, int32_t *cell, int32_t *face,
                                int32_t *boundary_id, double *xi, double *jinv, double *normal, double *jxw,
                                double *xq);

/* ------------------------------------------------------------------------------------------
 * Drop-in I/O surface, host side.
 * Parameter files: deal.II ParameterHandler text (`subsection`/`end`, `set key = value`, `#`
 * comments, `\` continuation) as read by Parameters::*::parse_parameters (source/core/
 * parameters.cc) and BoundaryConditions (boundary_conditions.h:130-425). Entries are addressed
 * "subsection/subsection/key" with deal.II's whitespace normalisation.
 * ------------------------------------------------------------------------------------------ */
typedef struct gls_prm gls_prm;
int gls_prm_parse(const char *text_or_path, int is_path, gls_prm **out);
int gls_prm_get(const gls_prm *prm, const char *path, char *buf, int cap); /* length, or GLS_ENOTFOUND */
int gls_prm_n_entries(const gls_prm *prm);
int gls_prm_entry(const gls_prm *prm, int i, char *path, int path_cap, char *value, int value_cap);
void gls_prm_destroy(gls_prm *prm);

/* Function expressions: deal.II Functions::ParsedFunction / FunctionParser over muParser
 * ("Function expression" = ';'-separated components, "Function constants" = "a=1, b=2",
 * variables "x,y,z,t"; pi/Pi predefined; deal.II's extra functions if/int/ceil/floor/cot/csc/
 * sec/pow/erfc and log = natural log). out[p*n_comp + c], values[p*n_vars + v] (HOST arrays). */
typedef struct gls_expr gls_expr;
int gls_expr_create(const char *expr, const char *vars, const char *constants, gls_expr **out);
int gls_expr_n_components(const gls_expr *e);
int gls_expr_eval(const gls_expr *e, int64_t n_points, const double *values, double *out);
void gls_expr_destroy(gls_expr *e);
/* The same on the DEVICE: values and out are DEVICE arrays with the layouts of gls_expr_eval, the launch is queued
 * on hip_stream (a hipStream_t; NULL: the default stream). One lane per point interprets the expression's stack
 * bytecode with the semantics of gls_expr_eval, operation by operation: + - * unary minus, comparisons, && || !,
 * ?:, abs floor ceil rint int sign, min max sum, constants and variables give the host's bits; / sqrt ^ pow and the
 * transcendental functions are the device math library's (within a few ulp of the host's). The operand stack
 * lives in LDS and holds 16 entries: a more deeply nested expression is GLS_EINVAL with a message, before any
 * launch. The device copy of the program is made at the first call (not thread-safe for one expression) and
 * released by gls_expr_destroy. Two calls on the same input are bitwise equal. */
int gls_expr_eval_device(const gls_expr *e, int64_t n_points, const double *values, double *out, void *hip_stream);

/* The L2 error of a DEVICE solution vector against an analytical solution on the device (the reference's
 * calculate_L2_error, navier_stokes_base.cc:887): QGauss(k+2) on every cell of the context, the exact solution
 * `exact` (variables: the dim coordinates, then t; components: the dim velocity components and optionally the
 * pressure -- without it the exact pressure is 0) evaluated by the device interpreter at the mapped points and at
 * `time`. Pass 1 sums int p_h, int p and the volume (box meshes: sum of JxW; mapped meshes: the sum of the Q1 cell
 * measures, GridTools::volume), pass 2 takes the two means from it:
 *   out[0] = sqrt(int |u_h - u|^2), out[1] = sqrt(int ((p_h - mean p_h) - (p - mean p))^2)   (HOST, one download).
 * gls_error_plan_create uploads the geometry the Gauss points need (box cells: cell_x0 / cell_h; mapped cells:
 * cell_support) and the 1D tables at the Gauss abscissae; mesh must be the description the context was created
 * from (dim, k, kp, n_cells and map_degree are checked); rebuild the plan after an adaptation. `exact` must
 * outlive the plan. Every layout of a context: brick, per-cell box, mapped, with hanging lines (the vector holds
 * the constrained values). The work is queued on the context's stream; per-block partials, then one ordered stage:
 * no atomics, two calls on the same input are bitwise equal. Kernels exist for dim 2, 3 and (k, kp) in {(1,1),
 * (2,1), (2,2)}, box and mapped (map_degree <= 3); anything else (2D Q3), an expression whose stack is deeper than
 * the interpreter's, a wrong variable count, fewer than dim components or a distributed context is GLS_EINVAL at
 * gls_error_plan_create. */
typedef struct gls_error_plan gls_error_plan;
int gls_error_plan_create(gls_ctx *ctx, const gls_mesh_desc *mesh, const gls_expr *exact, gls_error_plan **plan);
int gls_error_plan_destroy(gls_error_plan *plan);
int gls_l2_error(gls_ctx *ctx, gls_error_plan *plan, const double *sol, double time, double out[2]);

/* The L2 projection of a function onto the velocity-pressure space on the device (the reference's
 * set_initial_condition(L2projection): assemble_L2_projection + solve_system_GMRES(.., 1e-15, 1e-15),
 * gls_navier_stokes.cc:795-803, 830-914): the consistent mass matrix M (block diagonal per component, QGauss(k+1))
 * is never assembled. One launch per product integrates the cells' values back to their nodes by sum factorization
 * and writes element vectors; one ordered gather sums every node's slots in ascending cell order (no atomics).
 * gls_projection_plan_create uploads the geometry (box cells: cell_x0 / cell_h; mapped cells: cell_support), the 1D
 * tables, the node -> (cell, slot) incidence, and computes the diagonal of M (one launch); mesh must be the
 * description the context was created from (dim, k, kp, n_cells and map_degree are checked); rebuild the plan after
 * an adaptation. Every layout of a conforming context (brick, per-cell box, mapped, periodic: identified nodes are
 * one id) gives the same bits. Kernels exist for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}, box and mapped
 * (map_degree <= 3); anything else (2D Q3), a distributed context and a context with hanging or slip lines
 * (gls_set_hanging) are GLS_EINVAL at gls_projection_plan_create, with the limit named in gls_last_error().
 *   gls_mass_apply:     y = M x on DEVICE vectors in the context's DoF layout, no constraint mask (x != y)
 *   gls_mass_diagonal:  d = diag(M), the diagonal gls_l2_projection preconditions with (DEVICE vector)
 *   gls_l2_projection:  x = the L2 projection of f(x, t) at `time` (variables: the dim coordinates, then t; exactly
 *                       dim + 1 components u.., p; anything else is GLS_EINVAL), with the context's Dirichlet set
 *                       (gls_set_dirichlet) held fixed at its values, which is what distribute_local_to_global with
 *                       nonzero_constraints and distribute() yield. Jacobi-preconditioned conjugate gradients in
 *                       FP64 on the context's stream, from the Dirichlet values and zero elsewhere, on the free
 *                       rows, until |r| <= 1e-15 |b|; at most 10000 iterations, GLS_ENOCONV with the count in
 *                       gls_last_error() otherwise (info is filled either way). The right-hand side is integrated
 *                       on the device from the expression's bytecode at the Gauss points (gls_expr_eval_device's
 *                       interpreter and stack limit). Two calls on the same input are bitwise equal. Synchronizes
 *                       the stream (two scalar read-backs per iteration). */
typedef struct gls_projection_plan gls_projection_plan;
typedef struct { int iterations; double relative_residual; } gls_projection_info;
int gls_projection_plan_create(gls_ctx *ctx, const gls_mesh_desc *mesh, gls_projection_plan **plan);
int gls_projection_plan_destroy(gls_projection_plan *plan);
int gls_mass_apply(gls_ctx *ctx, gls_projection_plan *plan, const double *x, double *y);
int gls_mass_diagonal(gls_ctx *ctx, gls_projection_plan *plan, double *d);
int gls_l2_projection(gls_ctx *ctx, gls_projection_plan *plan, const gls_expr *f, double time, double *x,
                      gls_projection_info *info);

/* Output: NavierStokesBase::write_output_results (navier_stokes_base.cc:998-1086) — one patch per
 * cell with `subdivision` intervals (Lagrange cells when k > 1), point data velocity, pressure,
 * subdomain, vorticity, q_criterion [, velocity_eulerian when mesh->srf]; solution is a HOST
 * vector in this library's layout. Master records: write_vtu_and_pvd (solutions_output.cc:14-59). */
int gls_vtu_write(const char *filename, const gls_mesh_desc *mesh, const double *solution, int subdivision,
                  int subdomain, int binary);
int gls_pvtu_write(const char *filename, int dim, int srf, int n_pieces, const char *const *piece_files);
int gls_pvd_write(const char *filename, int n, const double *times, const char *const *files);

/* ------------------------------------------------------------------------------------------
 * Profiling hooks: time the next operator launches on the context stream with HIP events.
 * ------------------------------------------------------------------------------------------ */
int gls_timing_reset(gls_ctx *ctx);
/* which: 0 residual, 1 jacobian_apply, 2 diagonal, 3 J.v linearization (once per state),
 * 4 FP32 J.v of the mixed-precision V-cycle, 5 brick-surface slab sums (after each brick launch);
 * returns total ms and launch count */
int gls_timing_get(gls_ctx *ctx, int which, double *total_ms, int64_t *count);
int gls_timing_enable(gls_ctx *ctx, int enable);

#ifdef __cplusplus
}
#endif
#endif
