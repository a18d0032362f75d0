// gls_launch.hpp — host-side launch entry points of the device kernels.
#pragma once
#include "gls_common.hpp"

namespace gls {

// deterministic scatter of the per-cell kernels' element vectors (P.ev): y = per-node sums in slot order
hipError_t gather_element_vectors(double *y, const double *ev, const int64_t *voff, const int64_t *vslot, int64_t nv,
                                  const int64_t *poff, const int64_t *pslot, int64_t np, int dim, hipStream_t s);
hipError_t launch_cell_kernel(int dim, int k, int kp, int nq1d, int mode, const OpParams &P, const Tables1D &T,
                              hipStream_t s);
bool cell_kernel_supported(int dim, int k, int kp, int nq1d);
// sum-factorized J.v of 3D Q2-Q1 / Q2-Q2 cells from the linearization cache (gls_cell_sf.hip); hipErrorNotSupported
// when the launch is not its case (launch_cell_kernel then runs the dense kernel). GLS_CELL_SF=0: dense (A/B, tests)
hipError_t launch_cell_sf_jv(int dim, int k, int kp, int nq1d, const OpParams &P, const Tables1D &T, hipStream_t s);
bool cell_sf_enabled();
int cell_kernel_cells_per_block(int dim, int k, int nq1d, bool probe = false);  // cells per workgroup
// sum-factorized 3D Qk-Qk kernels on 2x2x2 Morton bricks (residual, J.v); k in {1,2}
hipError_t launch_brick_kernel(int k, int mode, const OpParams &P, const Tables1D &T, hipStream_t s);
size_t brick_qdata_size(int k, int n_cells);  // doubles of MODE_LIN storage
// J.v in FP32 arithmetic from P.qdf (FP32 linearization); v, y FP64 (multigrid smoother operator)
hipError_t launch_brick_jv_f32(int k, const OpParams &P, const Tables1D &T, hipStream_t s);
hipError_t vec_to_f32(const double *a, float *b, int64_t n, hipStream_t s);
hipError_t vec_from_f32(const float *a, double *b, int64_t n, hipStream_t s);
// Q2 brick J.v in the pencil dataflow (gls_brick_pencil.hip; FP64 from P.qd or FP32 from P.qdf), same
// contract as the lane-per-point MODE_JVQ launch with a slab; hipErrorNotSupported when not applicable
// (probing, colored launches, no slab). GLS_PENCIL=0 disables it.
hipError_t launch_pencil_jv(const OpParams &P, const Tables1D &T, hipStream_t s, bool f32);
// FP32 J.v of the V-cycle's residual with the restriction to the next-coarser nested level inside the
// kernel (hyper_cube, Morton bricks): rb - A v per brick, restricted 5 -> 3 per axis, as coarse element
// vectors [brick][27][4] (FP64) in P.slab's buffer; nothing goes to y. hipErrorNotSupported when not applicable
hipError_t launch_pencil_jv_restrict(const OpParams &P, const Tables1D &T, hipStream_t s);
// FP32 J.v of the V-cycle's first post-sweep with the prolongation from the next-coarser nested level inside the
// kernel (hyper_cube, Morton bricks): the fused damped-Jacobi sweep (P.jx) starts from x + P xc (P.pxc, coarse
// lattice of P.cube_nb1 cells per direction); x + P xc at the brick-surface nodes goes to P.pxp, which the slab
// sum that follows takes as its start values. hipErrorNotSupported when not applicable
hipError_t launch_pencil_jv_prolong(const OpParams &P, const Tables1D &T, hipStream_t s);
hipError_t launch_pencil_residual(const OpParams &P, const Tables1D &T, hipStream_t s);  // MODE_RESIDUAL, FP64
hipError_t launch_pencil_lin(const OpParams &P, const Tables1D &T, hipStream_t s);  // MODE_LIN (+ diagonal into P.y)
// MODE_RESLIN: residual (res_y / res_slab) + linearization (qd, qdf) + diagonal (y / slab) in one pass
hipError_t launch_pencil_reslin(const OpParams &P, const Tables1D &T, hipStream_t s);
hipError_t launch_pencil_ev(int mode, const OpParams &P, const Tables1D &T, hipStream_t s, bool f32 = false);  // forest sibling-group bricks -> element vectors
bool pencil_enabled();
bool cube_gather_enabled();  // GLS_CUBE_GATHER (read per launch): the pencil kernels' lattice gather, OpParams::cube_gather
// persistent wave-per-brick versions (gls_brick_wave.hip), selected by the launchers above
hipError_t launch_brick_wave(int k, int mode, const OpParams &P, const Tables1D &T, hipStream_t s);
hipError_t launch_brick_wave_jv_f32(int k, const OpParams &P, const Tables1D &T, hipStream_t s);
hipError_t launch_brick_wave_probe(int k, const OpParams &P, const Tables1D &T, int64_t j0, int nprobe, hipStream_t s);
size_t brick_wave_qdata_size(int k, int n_cells);

int brick_boundary_nodes(int k);  // NBND: brick-lattice nodes on the 2x2x2 brick's surface
// y[nodes[i]] = sum_{j in [off[i], off[i+1])} slab[slots[j]] (4 fields per node)
hipError_t brick_slab_sum(const double *slab, const int32_t *nodes, const int32_t *off, const int32_t *slots,
                          int64_t n_sum, int64_t n_vnodes, double *y, hipStream_t s);
// the same with an FP32 slab (slabf != nullptr) and/or a fused damped-Jacobi sweep (jb != nullptr:
// y holds x and is updated x <- x + jomega (jb - A x) / jd, rows in vmask use (A x)_i = jd_i x_i)
hipError_t brick_slab_sum_ex(const double *slab, const float *slabf, const int32_t *nodes, const int32_t *off,
                             const int32_t *slots, int64_t n_sum, int64_t n_vnodes, double *y, const uint8_t *vmask,
                             const double *jb, const double *jd, double jomega, hipStream_t s,
                             const double *rb = nullptr);  // rb (no jb): y = rb - A x
// the same sums on the structured hyper_cube (nb1 bricks per direction, lexicographic nodes, Morton
// bricks, no periodic wrap): slots computed from the lattice coordinates, no index arrays
hipError_t brick_slab_sum_cube(int k, int nb1, const double *slab, const float *slabf, int64_t n_vnodes, double *y,
                               const uint8_t *vmask, const double *jb, const double *jd, double jomega, hipStream_t s,
                               const double *rb = nullptr, double *x0 = nullptr,  // x0: OpParams::jx0's surface nodes
                               const double *xs = nullptr);  // xs (k = 2, with jb): the sweep's start values instead
                                                             //   of y's (launch_pencil_jv_prolong's OpParams::pxp)
// the same sums on the open subdivided hyper_rectangle (nb[a] bricks per axis, lexicographic nodes, bricks in
// tile-Morton order with tiles of s^3 bricks, s a power of two dividing every nb[a]; gls_box_mesh.hpp)
hipError_t brick_slab_sum_box(int k, const int nb[3], int s, const double *slab, const float *slabf, int64_t n_vnodes,
                              double *y, const uint8_t *vmask, const double *jb, const double *jd, double jomega,
                              hipStream_t st, const double *rb = nullptr, double *x0 = nullptr);
// coarse right-hand side from the bricks' restricted residuals (launch_pencil_jv_restrict: ev [brick][27][4],
// nb1 fine bricks = coarse cells per direction): bc[node] = sum of the node's <= 8 element-vector entries in
// ascending (Morton brick, local node) order, rows in the coarse vmask zeroed; n_vnodes = (2 nb1 + 1)^3.
// x0 (with the coarse diagonal d): x0 = 0 + omega bc / d stored too, mg_jacobi_update's first sweep from 0
hipError_t brick_restrict_sum_cube(int nb1, const double *ev, int64_t n_vnodes, double *bc, const uint8_t *vmask,
                                   hipStream_t s, double *x0 = nullptr, const double *d = nullptr, double omega = 0.0);
bool brick_fused_jacobi_supported(int k);  // the selected brick kernel honours OpParams::jx and ::slabf
// batched probing: Y[(j - j0) * n_dofs + i] += (J_cell-sum e_j)_i for nprobe unit vectors (MODE_JVQ)
bool brick_colors_supported(int k);  // colored brick launches (OpParams::bricks) available
bool brick_subset_supported(int k);  // brick-subset launches (OpParams::subset) available
hipError_t launch_brick_probe(int k, const OpParams &P, const Tables1D &T, int64_t j0, int nprobe, hipStream_t s);

// ---- BLAS-1 style kernels on device vectors (gls_vector_kernels.hip)
hipError_t vec_fill(double *x, int64_t n, double a, hipStream_t s);
hipError_t vec_copy(double *y, const double *x, int64_t n, hipStream_t s);
hipError_t vec_axpy(double *y, double a, const double *x, int64_t n, hipStream_t s);          // y += a x
hipError_t vec_axpby(double *y, double a, const double *x, double b, int64_t n, hipStream_t s);  // y = a x + b y
hipError_t vec_scale(double *x, double a, int64_t n, hipStream_t s);
hipError_t vec_div(double *y, const double *x, const double *d, int64_t n, hipStream_t s);       // y = x / d
// partial dot products: out[k] = sum_i A[k][i] * w[i] for k < nk (A rows have stride lda),
// written as per-block partials into work, reduced into out (device) by a second kernel.
hipError_t vec_multidot(const double *A, int64_t lda, int nk, const double *w, int64_t n, double *out,
                        double *work, hipStream_t s);
hipError_t vec_multidot2(const double *A, int64_t lda, int nk, const double *w, int64_t n1, int64_t off2, int64_t n2,
                         double *out, double *work, hipStream_t s);  // sums over [0,n1) U [off2, off2+n2)
// ghost exchange packing: buf[j*4 + {0,1,2,3}] <-> (vel comps, pressure) of local node nodes[j]
hipError_t vec_pack_nodes(const double *x, const int32_t *nodes, int64_t m, int64_t voff, double *buf, hipStream_t s);
hipError_t vec_unpack_nodes(double *x, const int32_t *nodes, int64_t m, int64_t voff, const double *buf, int add,
                            hipStream_t s);
// w -= sum_k h[k] * A[k]  (h on device); zero_init: w starts at 0 (not read)
hipError_t vec_multiaxpy(double *w, const double *A, int64_t lda, int nk, const double *h, double sign, int64_t n,
                         hipStream_t s, bool zero_init = false);
// w = y + a x
hipError_t vec_waxpy(double *w, const double *y, double a, const double *x, int64_t n, hipStream_t s);
// w -= sign * sum_k h[k] A[k] (nk <= 8, h on device), fused with out[k] = A[k] . w_new (k < nk, when
// dots) and out[dots ? nk : 0] = ||w_new||^2, both over the owned rows [0, n1) U [off2, off2 + n2).
// x0 (with d): x0 = 0 + omega w_new / d too, mg_jacobi_update's first sweep from 0 on w_new (in the same pass by the
// 16-byte kernel with dots, else by that update launched after it)
hipError_t vec_multiaxpy_dots(double *w, const double *A, int64_t lda, int nk, const double *h, double sign, int64_t n,
                              int64_t n1, int64_t off2, int64_t n2, bool dots, double scale, double *out,
                              double *work, hipStream_t s, double *x0 = nullptr, const double *d = nullptr,
                              double omega = 0.0);
// hanging-node constraint lines (CSR): distribute x[dof] = sum w src[master]; condense onto masters
hipError_t vec_csr_gather_set(double *x, const double *src, const int64_t *dof, const int64_t *off,
                              const int64_t *master, const double *w, int64_t n, hipStream_t s);
hipError_t vec_copy_gather_set(double *x, const double *v, const uint8_t *dmask, int64_t n, const int64_t *dof,
                               const int64_t *off, const int64_t *master, const double *w, int64_t nl, hipStream_t s);
hipError_t vec_csr_condense(double *y, const int64_t *tm, const int64_t *toff, const int64_t *tdof, const double *tw,
                            int64_t n, hipStream_t s);
hipError_t vec_csr_spmv(double *y, const double *x, const int64_t *off, const int32_t *col, const double *w, int64_t n,
                        bool add, hipStream_t s, int lanes = 1);  // y (+)= A x, CSR; lanes (1, 2, 4, 8, 16) per row
hipError_t vec_gather_scale_set(double *y, const double *d, const double *v, const int64_t *idx, int64_t m,
                                hipStream_t s, const double *rb = nullptr);  // y[idx] = d[idx]*v[idx] (rb: rb[idx] - d v)
// assembled-ILU helpers: x[idx] = a; val[ent] = y[row] (probe extraction; add: val[ent] += y[row]);
// a_ii <- r a_ii + sign(a_ii) t
hipError_t vec_set_const_indexed(double *x, const int32_t *idx, int64_t m, double a, hipStream_t s);
hipError_t csr_probe_extract(double *val, const int64_t *ent, const int32_t *row, int64_t m, const double *y,
                             hipStream_t s, bool add = false);
// dense column-major A (n x n, A[j * n + i] = A_ij, DoF numbering) from the ILU's probed CSR (rows / columns
// in its renumbered order, perm: DoF -> row); inv (n ints, scratch) receives row -> DoF. A is not zeroed here
hipError_t csr_to_dense(double *A, const int64_t *rowp, const int32_t *col, const double *val, const int32_t *perm,
                        const int32_t *inv, int64_t n, hipStream_t s);
hipError_t vec_permute(double *out, const double *in, const int32_t *idx, int64_t n, int dir, hipStream_t s);
// batched probing of the per-cell operator (nb probe vectors at stride bs / ys, element vectors at evs;
// pid[e] = probe of entry e, p0 = the batch's first probe)
hipError_t probe_set_batched(double *V, int64_t n, const int32_t *dofs, const int32_t *pid, int p0, int64_t m,
                             hipStream_t s);
hipError_t probe_extract_batched(double *val, const int64_t *ent, const int32_t *row, const int32_t *pid, int p0,
                                 int64_t m, const double *Y, int64_t n, hipStream_t s);
hipError_t vec_csr_gather_set_b(double *x, const int64_t *dof, const int64_t *off, const int64_t *master,
                                const double *w, int64_t n, int nb, int64_t bs, hipStream_t s);
hipError_t vec_csr_condense_b(double *y, const int64_t *tm, const int64_t *toff, const int64_t *tdof, const double *tw,
                              int64_t n, int nb, int64_t bs, hipStream_t s);
hipError_t vec_gather_scale_set_b(double *y, const double *d, const double *v, const int64_t *idx, int64_t m, int nb,
                                  int64_t bs, hipStream_t s);
hipError_t gather_element_vectors_b(double *y, const double *ev, const int64_t *voff, const int64_t *vslot, int64_t nv,
                                    const int64_t *poff, const int64_t *pslot, int64_t np, int dim, int nb, int64_t ys,
                                    int64_t evs, const uint8_t *act, int64_t el, int cb, int nblk, hipStream_t s);
// multicolor ILU triangular solves (gls_ilu_kernels.hip): y = L^-1 b, x = U^-1 y on node groups of <=
// kMaxGroupRows rows, colors in order (forward) / reverse order (backward)
constexpr int kMaxGroupRows = 4;
// multicolor ILU numeric factorization in place (same structures; rows of <= kIluMaxRow entries)
constexpr int kIluMaxRow = 640;
// the compact factorization (four workgroups per CU instead of three): rows of <= kIluCompactRow entries (Q2-Q1 3D
// cells of vertex valence <= 8: <= 402). Either needs fewer than 2^35 entries in all.
constexpr int kIluCompactRow = 448;
hipError_t ilu_mc_factor(const int32_t *grow, const int32_t *color_groups, int n_colors, const int64_t *rowp,
                         const int32_t *col, double *val, const int64_t *lsp, const int64_t *didx, double boost_tol,
                         double boost_val, const int64_t *moff, const uint16_t *map, bool compact, double *rdiag,
                         hipStream_t s);  // rdiag (n): 1 / U_ii, written row by row (read for the later colors' pivots)
// the factorization's row-position map (map == nullptr in ilu_mc_factor: column searches instead)
hipError_t ilu_mc_factor_map(int64_t n, const int64_t *rowp, const int32_t *col, const int64_t *lsp,
                             const int64_t *didx, const int64_t *moff, uint16_t *map, hipStream_t s);
// per node group (int64): r0, nr, rowp[r0], rowp[r0 + nr], rowp[r0 + 1..3] (INT64_MAX past nr), 0, lsp[4],
// usp[4], didx[4], rowp[r0 + 1..4] (the solves' group descriptor)
constexpr int kGroupDesc = 24;
hipError_t ilu_mc_solve(const int64_t *gdesc, const int32_t *color_groups, int n_colors, const int32_t *col,
                        const double *val, const double *b, double *y, double *x, const uint8_t *waves_lower,
                        const uint8_t *waves_upper, hipStream_t s);
hipError_t vec_pack_dofs(const double *x, const int32_t *dofs, int64_t m, double *buf, hipStream_t s);
hipError_t vec_unpack_dofs(double *x, const int32_t *dofs, int64_t m, const double *buf, hipStream_t s);
hipError_t vec_add_dofs_ordered(double *x, const int32_t *u, const int32_t *off, const int32_t *slot, int64_t n,
                                const double *buf, hipStream_t s);
hipError_t vec_add_nodes_ordered(double *x, const int32_t *u, const int32_t *off, const int32_t *slot, int64_t n,
                                 int64_t voff, const double *buf, hipStream_t s);  // 4 values per node slot
hipError_t csr_diag_perturb(double *val, const int64_t *didx, int64_t n, double athresh, double rthresh, hipStream_t s);
hipError_t vec_set_const_indexed64(double *x, const int64_t *idx, int64_t m, double a, hipStream_t s);
// x[u[i]] += sum of buf[slot[j]] over j in [off[i], off[i+1]) in order (u: 64-bit positions, the ILU's remote entries)
hipError_t vec_add_pos_ordered(double *x, const int64_t *u, const int32_t *off, const int32_t *slot, int64_t n,
                               const double *buf, hipStream_t s);
hipError_t vec_set_indexed(double *y, const int64_t *idx, const double *vals, int64_t m, hipStream_t s);  // y[idx]=vals (vals null -> 0)
int multidot_work_size();

// ---- Kelly error indicator (gls_kelly.hip): 1D tables of the selected space at the face rule
struct KellyTables {
  int nq;                             // face quadrature points per direction
  double w[kMaxQ1D];                  // Gauss weights on [0, 1]
  double V[kMaxQ1D][kMaxNodes1D];     // basis values at the face points
  double De[2][kMaxNodes1D];          // basis derivatives at xi = 0 and xi = 1
  double xq[kMaxQ1D];                 // Gauss points on [0, 1]
  double xn[kMaxNodes1D];             // support points (Gauss-Lobatto) of the basis
};
// face-list form for meshes with hanging faces: fint[e] = int over the piece of face e of
// sum_c [d_n u_c]^2, the piece being rect_a / rect_b in the reference coordinates of cell fa[e]
// (its face xi_d = 1) and fb[e] (its face xi_d = 0), d = fdir[e]; QGauss(T.nq)^(dim-1) on the piece
hipError_t launch_kelly_faces(int dim, int m, const int32_t *cell_nodes, const double *geo, const double *sol,
                              int64_t n_faces, const int32_t *fa, const int32_t *fb, const int32_t *fdir,
                              const double *rect_a, const double *rect_b, int ncomp, int64_t base, int stride,
                              const KellyTables &T, double *fint, hipStream_t s);
// mapped meshes: per piece e and face point q, xi / g [e][q][side][dim] (g = J^-1 n), jxw [e][q]
hipError_t launch_kelly_mapped(int dim, int m, const int32_t *cell_nodes, const double *sol, int64_t n_pieces, int nqf,
                               const int32_t *ca, const int32_t *cb, const double *xi, const double *g,
                               const double *jxw, int ncomp, int64_t base, int stride, const KellyTables &T,
                               double *fint, hipStream_t s);
// eta[cell] = sqrt(sum over faces with nbr >= 0 of diam/24 * int_F sum_c [d_n u_c]^2); component c of
// node n at sol[base + n * stride + c], c < ncomp; cell_nodes [n_cells][(m+1)^dim]; nbr [n_cells][2 dim]
hipError_t launch_kelly(int dim, int m, const int32_t *cell_nodes, const int32_t *nbr, const double *geo,
                        const double *sol, int n_cells, int ncomp, int64_t base, int stride, const KellyTables &T,
                        double *eta, hipStream_t s);

// ---- boundary forces and torques (gls_boundary.hip): every boundary in one pass. Per face point
// pt = face * nqf + q: xi / normal / xq [pt][dim], jinv [pt][dim][dim] (d xi_a / d x_i), jxw [pt];
// per face its cell and its slot (row of the tables, -1: skipped); cor [n_slots][3]. The velocity of
// node n is at sol[n * dim + c], the pressure of node n at sol[pbase + n]. partial:
// boundary_loads_blocks(n_pts) * n_slots * 6 doubles; out [n_slots][6] = f_x f_y f_z T_x T_y T_z, summed in a
// fixed order (bitwise reproducible). Instantiated for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}.
int64_t boundary_loads_blocks(int64_t n_pts);
bool boundary_loads_supported(int dim, int k, int kp);
hipError_t launch_boundary_loads(int dim, int k, int kp, const int32_t *cell_vnodes, const int32_t *cell_pnodes,
                                 const double *sol, int64_t pbase, int64_t n_pts, int nqf, const int32_t *fcell,
                                 const int32_t *fslot, const double *xi, const double *jinv, const double *normal,
                                 const double *jxw, const double *xq, double nu, const double *cor, int n_slots,
                                 double *partial, double *out, hipStream_t s);

// ---- flow diagnostics (gls_diagnostics.hip): CFL maximum, int 1/2 |u|^2, int 1/2 |curl u|^2 and the volume in
// one pass, one lane per cell, QGauss(k+1). geo [n_cells][4] (box extents), gq [n_cells][nq][kGeo] (mapped
// cells; nullptr: boxes), meas [n_cells] = cell->measure(), tab = V [k+1][k+1] | D [k+1][k+1] | w [k+1] (1D
// velocity basis values / derivatives [q][node] and Gauss weights). partial: flow_diagnostics_blocks(n_cells)
// * 4 doubles; out [4], folded in a fixed order (bitwise reproducible). Instantiated for dim 2, 3 and k 1, 2.
int64_t flow_diagnostics_blocks(int64_t n_cells);
bool flow_diagnostics_supported(int dim, int k, int kp);
hipError_t launch_flow_diagnostics(int dim, int k, const int32_t *cell_vnodes, const double *geo, const double *gq,
                                   const double *meas, const double *tab, const double *sol, int64_t n_cells, double dt,
                                   double *partial, double *out, hipStream_t s);

// ---- VTU point data (gls_output.hip): for every cell and every patch point of build_patches(mapping,
// subdivision) the position, velocity, pressure, vorticity, running-sum q_criterion and (srf) velocity_eulerian,
// in the VTU layout: point P = cell * npp + p, p x-fastest over the (subdivision+1)^dim lattice; pts / vel / eul
// [P][3], pre / qcr [P], vort [P][3] (3D) or [P] (2D). One lane per patch point, sum-factorized through LDS.
// x0h [n_cells][2 dim] = x0 | h (box cells, map_degree 0) or support [n_cells][(map_degree+1)^dim][dim]; tab =
// Vv [np1][k+1] | Dv | Vp [np1][kp+1] | Vm [np1][map_degree+1] | Dm (the last two for mapped cells only): the 1D
// bases and derivatives at t / subdivision. Instantiated for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}, box
// and mapped (map_degree <= 3); (subdivision+1)^dim <= 256.
bool output_fields_supported(int dim, int k, int kp, int map_degree, int subdivision);
hipError_t launch_output_fields(int dim, int k, int kp, int map_degree, int subdivision, const int32_t *cell_vnodes,
                                const int32_t *cell_pnodes, const double *sol, int64_t pbase, const double *x0h,
                                const double *support, const double *tab, int64_t n_cells, int srf, const double *omega,
                                double *pts, double *vel, double *pre, double *vort, double *qcr, double *eul,
                                hipStream_t s);

// ---- L2 error against an analytical solution (gls_error.hip): QGauss(k+2), one lane per quadrature point, the
// exact solution from the expression's program (gls_expr_device.hpp: variables x, y [, z], t; components u, v [, w]
// [, p]) at the mapped points and `time`. Two passes queued on s: out[0..2] = int p_h, int p, volume (volume >= 0
// replaces the sum of JxW), then out[3] = int |u_h - u|^2 and out[4] = int ((p_h - mean p_h) - (p - mean p))^2;
// out: 6 doubles, partial: l2_error_blocks(...) * 3 doubles, folded in a fixed order (bitwise reproducible).
// x0h / support as for the output fields; tab = Vv [k+2][k+1] | Vp [k+2][kp+1] | xq [k+2] | wq [k+2] | Vm
// [k+2][map_degree+1] | Dm (the last two for mapped cells only) at the Gauss abscissae. Instantiated for dim 2, 3
// and (k, kp) in {(1,1), (2,1), (2,2)}, box and mapped (map_degree <= 3); max_stack <= 16.
namespace expr {
struct DeviceProgram;
}
bool l2_error_supported(int dim, int k, int kp, int map_degree, int max_stack);
int64_t l2_error_blocks(int dim, int k, int kp, int map_degree, int max_stack, int64_t n_cells);
hipError_t launch_l2_error(int dim, int k, int kp, int map_degree, const int32_t *cell_vnodes, const int32_t *cell_pnodes,
                           const double *sol, int64_t pbase, const double *x0h, const double *support, const double *tab,
                           int64_t n_cells, const expr::DeviceProgram &exact, double time, double volume, double *partial,
                           double *out, hipStream_t s);

// ---- the consistent mass matrix, matrix-free (gls_mass.hip): QGauss(k+1), one lane per quadrature point, the dim
// velocity components and the pressure as scalar fields. One launch writes the element vectors ev [n_cells][NV dim +
// NP] in the per-cell kernels' layout (gather_element_vectors sums them per node in a fixed order): kMassApply
// M_e x_e of the device vector x, kMassRhs int phi f(x, time) JxW with f's dim + 1 components from the device
// interpreter, kMassDiag sum_q phi_a(q)^2 JxW. x0h / support as for the output fields; tab = Vv [k+1][k+1] | Vp
// [k+1][kp+1] | xq [k+1] | wq [k+1] | Vv^2 | Vp^2 | Vm [k+1][map_degree+1] | Dm (the last two for mapped cells only)
// at the Gauss abscissae. Instantiated for dim 2, 3 and (k, kp) in {(1,1), (2,1), (2,2)}, box and mapped
// (map_degree <= 3); max_stack <= 16 (0: no expression).
constexpr int kMassApply = 0, kMassRhs = 1, kMassDiag = 2;
bool mass_supported(int dim, int k, int kp, int map_degree, int max_stack);
hipError_t launch_mass(int mode, int dim, int k, int kp, int map_degree, const int32_t *cell_vnodes,
                       const int32_t *cell_pnodes, const double *x, int64_t pbase, const double *x0h,
                       const double *support, const double *tab, int64_t n_cells, const expr::DeviceProgram *f,
                       double time, double *ev, hipStream_t s);

// ---- geometric multigrid (gls_mg_kernels.hip): nested Qk node lattices (boxes), k <= 2
hipError_t mg_inject(const double *fine, double *coarse, const int nf[3], const int nc[3], hipStream_t s);
// one-pass 3D transfer with per-axis tap tables [n_out][5] (index, weight) and tap counts [n_out]
hipError_t mg_transfer3d(const double *in, double *out, const int nin[3], const int nout[3],
                         const int32_t *const taps[3], const double *const w[3], const int32_t *const cnt[3],
                         hipStream_t s);
// two-pass transfer (LDS-tiled xy pass + z pass); work holds 4 * (xy of the smaller lattice) * (z of the
// larger) doubles. tile_fits: host check that a per-axis tap table (axis 0/1) fits the kernel's tiles.
hipError_t mg_transfer_2pass(const double *in, double *out, const int nin[3], const int nout[3], int restrict_,
                             const int32_t *const taps[3], const double *const w[3], const int32_t *const cnt[3],
                             double *work, hipStream_t s, int add = 0, int wrap = 0);  // add (prolongation): out += P in
// wrap: a lattice with periodic axes, whose tap tables hold unwrapped indices at the seam (gls_mg_attach_periodic)
int mg_transfer_tile_fits(int restrict_, int axis, int n_out, const int32_t *taps, const int32_t *cnt);
hipError_t mg_box_gather(const double *loc, double *box, const int32_t *map, int64_t nbox, int64_t nvl,
                         int64_t n_owned, hipStream_t s);  // n_owned < 0: all nodes
hipError_t mg_box_scatter(const double *box, double *loc, const int32_t *map, int64_t nbox, int64_t nvl,
                          hipStream_t s);
// coarsest-level direct solve: invert the probed matrix (Y column-major) into aug = [I | A^-1]
hipError_t mg_dense_invert(const double *Y, double *aug, int n, int *status, hipStream_t s);  // status: dropped columns
hipError_t mg_unit_step(double *e, int64_t j, hipStream_t s);  // e[j-1] = 0, e[j] = 1
// probed columns: constrained rows of column j become D_c(j) delta_ij (gls_jacobian_apply's rule)
hipError_t mg_probe_fix(double *Y, int64_t n, int64_t j0, int nprobe, const int64_t *con, int64_t ncon, const double *d,
                        hipStream_t s);
hipError_t mg_dense_apply(const double *aug, int n, const double *b, double *x, hipStream_t s);
// column-major n x n: row / column `pin` -> identity; zero one row (the LU path's gauge pin)
hipError_t mg_pin_dof(double *A, int64_t n, int64_t pin, hipStream_t s);
hipError_t mg_zero_row(double *A, int64_t n, int64_t row, hipStream_t s);
// x <- (LU)^-1 x for a dense FP32 LU factor without pivoting (column-major, lda = n; gls_mg_kernels.hip)
hipError_t dense_lu_solve_f32(const float *LU, int n, float *x, hipStream_t s, int bl = -1, int bu = -1);  // bl / bu: bandwidths (-1 dense)
hipError_t mg_jacobi_update(double *x, const double *b, const double *y, const double *d, double omega, int64_t n,
                            int zero_start, hipStream_t s);

// additive cell-Vanka smoother on 3D Q2-Q1 / Q2-Q2 per-cell contexts (gls_vanka.hip). nd = 89 / 108 DoFs per cell;
// the FP32 inverses are [n_cells][nd][vanka_row_floats(nd)] (rows padded to 16 bytes).
int vanka_row_floats(int nd);
// K [n_cells][nd][nd]: the element Jacobians from the linearization cache P.cq (cq_mode 2), unconstrained
hipError_t launch_vanka_element(int kp, const OpParams &P, const Tables1D &T, double *K, hipStream_t s);
// A [n_cells][nd][nd]: K summed over each cell's neighbours through the overlap maps (gls_vanka_maps.hpp); DoFs with
// con[dof] != 0 become rows / columns of the identity times diag[dof]
hipError_t launch_vanka_patch(int n_cells, int nd, const double *K, const int64_t *nb_off, const int32_t *nb_cell,
                              const int64_t *ov_off, const uint8_t *ov_i, const uint8_t *ov_j, const int32_t *cell_dofs,
                              const uint8_t *con, const double *diag, double *A, hipStream_t s);
// Ainv = A^-1 per cell (FP64 Gauss-Jordan with partial pivoting, stored FP32); flag[cell] = 1 (never cleared here) where
// a pivot is zero or not finite or the inverse overflows FP32
hipError_t launch_vanka_invert(int n_cells, int nd, const double *A, float *Ainv, int32_t *flag, hipStream_t s);
// ev [n_cells][nd] = Ainv_c r[cell_dofs[c]]; then x[dof] += omega / (cells holding dof) * its slots' sum in cell order
hipError_t launch_vanka_apply(int n_cells, int nd, const float *Ainv, const int32_t *cell_dofs, const double *r, double *ev,
                              hipStream_t s);
hipError_t launch_vanka_update(double *x, const double *ev, const int64_t *voff, const int64_t *vslot, int64_t nv,
                               const int64_t *poff, const int64_t *pslot, int64_t np, int dim, double omega, hipStream_t s);

}  // namespace gls
