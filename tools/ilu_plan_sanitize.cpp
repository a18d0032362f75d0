// Stand-alone run of the host-only ILU plan (csrc/gls_ilu_plan.cpp) for the sanitizers: a 3x3x3 Q2-Q1 cube with
// no-slip walls and a few constraint lines, both orderings, fill 0 and 1, block-Jacobi, and the two-stage path of a
// distributed context (ghost nodes, two neighbour records). Exits 0 when every plan is a sorted pattern with its
// diagonals under a permutation.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o ilu_plan_sanitize
//       tools/ilu_plan_sanitize.cpp softx_2020_200_amd/csrc/gls_ilu_plan.cpp softx_2020_200_amd/csrc/gls_sparse.cpp
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/gls_native.h"
#include "../softx_2020_200_amd/csrc/gls_ilu_plan.hpp"

// the library's error setters (gls_api.cpp), which the plan's C export reports through
int gls_internal_set_err(int code, const char *msg) {
  std::fprintf(stderr, "error %d: %s\n", code, msg);
  return code;
}

static int check(const gls::IluPlan &P, const char *what) {
  const int64_t n = P.n;
  std::vector<char> seen((size_t)n, 0);
  for (int32_t r : P.perm)
    if (r < 0 || r >= n || seen[(size_t)r]++) return std::fprintf(stderr, "%s: perm\n", what), 1;
  for (int64_t r = 0; r < n; ++r) {
    const auto b = P.col.begin() + P.rowp[(size_t)r], e = P.col.begin() + P.rowp[(size_t)r + 1];
    if (!std::is_sorted(b, e) || P.col[(size_t)P.didx[(size_t)r]] != r) return std::fprintf(stderr, "%s: row %lld\n", what, (long long)r), 1;
  }
  for (int64_t t : P.pent)
    if (t < 0 || t >= (int64_t)P.col.size()) return std::fprintf(stderr, "%s: pent\n", what), 1;
  std::printf("%-28s n %lld nnz(A) %lld nnz %lld probes %d colors %d blocks %d mc_solve %d\n", what, (long long)n,
              (long long)P.nnz_a, (long long)P.col.size(), P.n_probes, P.n_order_colors, P.n_blocks, (int)P.mc_solve);
  return 0;
}

int main() {
  const int nc1 = 3, nv1 = 2 * nc1 + 1, np1 = nc1 + 1;
  gls::IluPlanInput in;
  in.dim = 3, in.k = 2, in.kp = 1;
  in.n_vnodes = nv1 * nv1 * nv1, in.n_pnodes = np1 * np1 * np1, in.n_cells = nc1 * nc1 * nc1;
  auto vnode = [&](int x, int y, int z) { return x + nv1 * (y + nv1 * z); };
  auto pnode = [&](int x, int y, int z) { return x + np1 * (y + np1 * z); };
  for (int k = 0; k < nc1; ++k)
    for (int j = 0; j < nc1; ++j)
      for (int i = 0; i < nc1; ++i) {
        for (int a = 0; a < 27; ++a) in.cell_vnodes.push_back(vnode(2 * i + a % 3, 2 * j + (a / 3) % 3, 2 * k + a / 9));
        for (int a = 0; a < 8; ++a) in.cell_pnodes.push_back(pnode(i + a % 2, j + (a / 2) % 2, k + a / 4));
      }
  const int64_t nvd = 3 * in.n_vnodes;
  for (int z = 0; z < nv1; ++z)
    for (int y = 0; y < nv1; ++y)
      for (int x = 0; x < nv1; ++x)
        if (x == 0 || y == 0 || z == 0 || x == nv1 - 1 || y == nv1 - 1 || z == nv1 - 1)
          for (int c = 0; c < 3; ++c) in.con_dofs.push_back(3 * vnode(x, y, z) + c);
  // lines: two velocity components between interior masters, one with a Dirichlet master, one pressure line
  const int64_t lines[4][3] = {{3 * vnode(3, 3, 3) + 0, 3 * vnode(2, 3, 3) + 0, 3 * vnode(4, 3, 3) + 0},
                               {3 * vnode(3, 2, 3) + 1, 3 * vnode(3, 1, 3) + 1, 3 * vnode(3, 3, 3) + 1},
                               {3 * vnode(1, 3, 3) + 2, 3 * vnode(0, 3, 3) + 2, 3 * vnode(2, 3, 3) + 2},
                               {nvd + pnode(1, 1, 1), nvd + pnode(0, 1, 1), nvd + pnode(2, 1, 1)}};
  in.h_off.push_back(0);
  for (const auto &l : lines) {
    in.h_dof.push_back(l[0]);
    in.h_master.push_back(l[1]);
    in.h_master.push_back(l[2]);
    in.h_off.push_back((int64_t)in.h_master.size());
    in.con_dofs.push_back(l[0]);
  }
  int bad = 0;
  std::string err;
  for (int ordering : {GLS_ILU_ORDER_CM, GLS_ILU_ORDER_MULTICOLOR})
    for (int fill : {0, 1})
      for (int64_t blk : {(int64_t)0, (int64_t)400}) {
        in.ordering = ordering, in.fill = fill, in.block_dofs = blk;
        gls::IluPlan P;
        if (gls::ilu_plan_patterns(in, P, err) != 0 || gls::ilu_plan_finish(in, {}, 0, P, err) != 0)
          return std::fprintf(stderr, "plan: %s\n", err.c_str()), 1;
        char what[64];
        std::snprintf(what, sizeof(what), "order %d fill %d block %lld", ordering, fill, (long long)blk);
        bad += check(P, what);
      }
  // a rank of a distributed context: the last nodes are ghosts; two entries arrive from a neighbour
  in.n_owned = in.n_vnodes - 20, in.n_owned_p = in.n_pnodes - 5;
  for (int ordering : {GLS_ILU_ORDER_CM, GLS_ILU_ORDER_MULTICOLOR}) {
    in.ordering = ordering, in.fill = 0, in.block_dofs = 0;
    gls::IluPlan P;
    if (gls::ilu_plan_patterns(in, P, err) != 0) return std::fprintf(stderr, "plan: %s\n", err.c_str()), 1;
    const int64_t i = 3 * vnode(1, 1, 1), j = 3 * vnode(5, 5, 2);
    const std::vector<gls::IluRemoteEntry> remote = {{0, 3, i, j}, {1, 7, i, j}, {1, 2, j, i}};
    if (gls::ilu_plan_finish(in, remote, 2, P, err) != 0) return std::fprintf(stderr, "plan: %s\n", err.c_str()), 1;
    bad += check(P, ordering ? "distributed multicolor" : "distributed cm");
    if (P.rr.size() != 3 || P.rr[2] != 3) bad += 1, std::fprintf(stderr, "remote lists\n");
  }
  // the C export on the same mesh
  in.n_owned = in.n_owned_p = -1;
  int64_t nnz = 0, nnz_a = 0;
  int npr = 0, mcs = 0;
  if (gls_ilu_plan(3, 2, 1, in.n_vnodes, in.n_pnodes, in.n_cells, in.cell_vnodes.data(), in.cell_pnodes.data(),
                   (int64_t)in.con_dofs.size(), in.con_dofs.data(), 4, in.h_dof.data(), in.h_off.data(), in.h_master.data(), 0,
                   GLS_ILU_ORDER_MULTICOLOR, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &nnz, &nnz_a, &npr, &mcs) != GLS_OK)
    return 1;
  std::vector<int32_t> perm((size_t)(nvd + in.n_pnodes)), rowp(perm.size() + 1), col((size_t)nnz), probe(perm.size()), color(perm.size());
  if (gls_ilu_plan(3, 2, 1, in.n_vnodes, in.n_pnodes, in.n_cells, in.cell_vnodes.data(), in.cell_pnodes.data(),
                   (int64_t)in.con_dofs.size(), in.con_dofs.data(), 4, in.h_dof.data(), in.h_off.data(), in.h_master.data(), 0,
                   GLS_ILU_ORDER_MULTICOLOR, 0, perm.data(), rowp.data(), col.data(), nnz, probe.data(), color.data(), &nnz, &nnz_a,
                   &npr, &mcs) != GLS_OK)
    return 1;
  std::printf("export: nnz %lld nnz(A) %lld probes %d mc_solve %d\n", (long long)nnz, (long long)nnz_a, npr, mcs);
  return bad ? 1 : 0;
}
