// gls_ilu_plan.cpp -- the host-only plan of gls_ilu_attach (gls_ilu_plan.hpp), and its C export gls_ilu_plan.
//
// The matrix's graph is the reference's system-matrix sparsity (make_sparsity_pattern with nonzero_constraints,
// keep_constrained_dofs = false, gls_navier_stokes.cc:208-211): a constrained row / column holds its diagonal only,
// lines (hanging nodes, slip on curved walls) couple their masters. It is probed with distance-2-colored unit
// vectors (no two DoFs of a probe share a row). The DoFs are renumbered like DoFRenumbering::Cuthill_McKee
// (gls_navier_stokes.cc:70), or in the multicolor order, and the level-of-fill pattern of ILU(fill) is inserted
// with explicit zeros.
#include "gls_ilu_plan.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <utility>

#include "../../include/gls_native.h"
#include "gls_error.hpp"
#include "gls_sparse.hpp"

namespace gls {
namespace {

int ipow_(int b, int e) {
  int r = 1;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}

int fail(std::string &err, const char *fmt, long long a = 0, long long b = 0) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b);
  err = buf;
  return -1;
}

// unified nodes: velocity nodes [0, nv), separate pressure nodes [nv, nv + np)
struct Layout {
  int dim, nvc, npc, ncn;
  bool sep, dist;
  int64_t nv, np, nc, n, nu, nvd, n_owned, n_owned_p;
  const int32_t *cv, *cp;
  explicit Layout(const IluPlanInput &in)
      : dim(in.dim), nvc(ipow_(in.k + 1, in.dim)), sep(!in.cell_pnodes.empty()), dist(in.n_owned >= 0),
        nv(in.n_vnodes), np(in.n_pnodes), nc(in.n_cells), n_owned(in.n_owned), n_owned_p(in.n_owned_p),
        cv(in.cell_vnodes.data()), cp(in.cell_pnodes.data()) {
    npc = sep ? ipow_(in.kp + 1, dim) : 0;
    ncn = nvc + npc;
    nvd = (int64_t)dim * nv;
    n = nvd + np;
    nu = nv + (sep ? np : 0);
  }
  int64_t cell_node(int64_t cell, int a) const {
    return a < nvc ? cv[(size_t)(cell * nvc + a)] : nv + cp[(size_t)(cell * npc + a - nvc)];
  }
  // DoFs of a unified node and their probe slot (component; dim = pressure)
  int node_dofs(int64_t x, int64_t *d, int *slot) const {
    if (x >= nv) { d[0] = nvd + (x - nv); slot[0] = dim; return 1; }
    int m = 0;
    for (int cc = 0; cc < dim; ++cc) { d[m] = x * dim + cc; slot[m++] = cc; }
    if (!sep) { d[m] = nvd + x; slot[m++] = dim; }
    return m;
  }
  // across ranks (Ifpack additive Schwarz, overlap 0, as the reference runs with MPI): each rank factors its owned
  // rows and columns; ghost DoFs are identity rows and drop out of the pattern
  bool ghost(int64_t d) const {
    if (!dist) return false;
    return d < nvd ? d / dim >= n_owned : d - nvd >= n_owned_p;
  }
};

// The cell-coupling pattern under a constraint view (cons: constrained DoFs; dir: those that drop out of the lines
// too -- Dirichlet DoFs, as in the closed AffineConstraints, and whatever else the view removes): an unconstrained
// DoF couples the effective DoFs of its cells, a constrained DoF only itself. Rows sorted.
void cell_pattern(const Layout &L, const IluPlanInput &in, const std::vector<int64_t> &lidx, const std::vector<char> &cons,
                  const std::vector<char> &dir, IluCsr &A) {
  const int64_t n = L.n, nc = L.nc;
  // effective DoFs of each cell: its unconstrained DoFs and the (non-Dirichlet) masters of its lines
  std::vector<int64_t> effoff((size_t)nc + 1, 0), eff, buf;
  for (int64_t e = 0; e < nc; ++e) {
    buf.clear();
    for (int a = 0; a < L.ncn; ++a) {
      int64_t d[4];
      int sl[4];
      const int m = L.node_dofs(L.cell_node(e, a), d, sl);
      for (int j = 0; j < m; ++j) {
        const int64_t li = lidx[(size_t)d[j]];
        if (li >= 0 && !dir[(size_t)d[j]]) {
          for (int64_t t = in.h_off[(size_t)li]; t < in.h_off[(size_t)li + 1]; ++t)
            if (!dir[(size_t)in.h_master[(size_t)t]]) buf.push_back(in.h_master[(size_t)t]);
        } else if (!cons[(size_t)d[j]]) {
          buf.push_back(d[j]);
        }
      }
    }
    std::sort(buf.begin(), buf.end());
    buf.erase(std::unique(buf.begin(), buf.end()), buf.end());
    eff.insert(eff.end(), buf.begin(), buf.end());
    effoff[(size_t)e + 1] = (int64_t)eff.size();
  }
  // DoF -> cells whose effective list holds it
  std::vector<int64_t> dcoff((size_t)n + 1, 0), dcell;
  for (int64_t d : eff) ++dcoff[(size_t)d + 1];
  for (int64_t i = 0; i < n; ++i) dcoff[(size_t)i + 1] += dcoff[(size_t)i];
  dcell.resize((size_t)dcoff[(size_t)n]);
  {
    std::vector<int64_t> f(dcoff.begin(), dcoff.end() - 1);
    for (int64_t e = 0; e < nc; ++e)
      for (int64_t t = effoff[(size_t)e]; t < effoff[(size_t)e + 1]; ++t) dcell[(size_t)f[(size_t)eff[(size_t)t]]++] = e;
  }
  A.off.assign((size_t)n + 1, 0);
  A.col.clear();
  std::vector<int64_t> stamp((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    buf.clear();
    buf.push_back(i);
    stamp[(size_t)i] = i;
    if (!cons[(size_t)i])
      for (int64_t t = dcoff[(size_t)i]; t < dcoff[(size_t)i + 1]; ++t) {
        const int64_t e = dcell[(size_t)t];
        for (int64_t u = effoff[(size_t)e]; u < effoff[(size_t)e + 1]; ++u) {
          const int64_t j = eff[(size_t)u];
          if (stamp[(size_t)j] != i) { stamp[(size_t)j] = i; buf.push_back(j); }
        }
      }
    std::sort(buf.begin(), buf.end());
    A.col.insert(A.col.end(), buf.begin(), buf.end());
    A.off[(size_t)i + 1] = (int64_t)A.col.size();
  }
}

// node graph of a pattern: x ~ y when a row of x holds a DoF of y (x itself included)
void node_graph(const Layout &L, const std::vector<int64_t> &dnode, const IluCsr &A, IluCsr &G) {
  const int64_t nu = L.nu;
  G.off.assign((size_t)nu + 1, 0);
  G.col.clear();
  std::vector<int64_t> stamp((size_t)nu, -1), buf;
  for (int64_t x = 0; x < nu; ++x) {
    buf.clear();
    buf.push_back(x);
    stamp[(size_t)x] = x;
    int64_t d[4];
    int sl[4];
    const int m = L.node_dofs(x, d, sl);
    for (int j = 0; j < m; ++j)
      for (int64_t t = A.off[(size_t)d[j]]; t < A.off[(size_t)d[j] + 1]; ++t) {
        const int64_t y = dnode[(size_t)A.col[(size_t)t]];
        if (stamp[(size_t)y] != x) { stamp[(size_t)y] = x; buf.push_back(y); }
      }
    std::sort(buf.begin(), buf.end());
    G.col.insert(G.col.end(), buf.begin(), buf.end());
    G.off[(size_t)x + 1] = (int64_t)G.col.size();
  }
}

// greedy colouring of a node graph: the nodes in `visit` order (nullptr: natural order) take the lowest colour no
// node within `distance` (1 or 2) edges holds. Returns the number of colours.
int greedy_coloring(const IluCsr &G, const int64_t *visit, int distance, std::vector<int> &color) {
  const int64_t nu = (int64_t)G.off.size() - 1;
  color.assign((size_t)nu, -1);
  std::vector<int> mark;
  int ncol = 0;
  auto mark_row = [&](int64_t z, int64_t x) {
    for (int64_t u = G.off[(size_t)z]; u < G.off[(size_t)z + 1]; ++u) {
      const int cy = color[(size_t)G.col[(size_t)u]];
      if (cy >= 0) {
        if ((int)mark.size() <= cy) mark.resize((size_t)cy + 1, -1);
        mark[(size_t)cy] = (int)x;
      }
    }
  };
  for (int64_t v = 0; v < nu; ++v) {
    const int64_t x = visit ? visit[v] : v;
    if (distance == 1) mark_row(x, x);
    else
      for (int64_t t = G.off[(size_t)x]; t < G.off[(size_t)x + 1]; ++t) mark_row(G.col[(size_t)t], x);
    int col = 0;
    while (col < (int)mark.size() && mark[(size_t)col] == (int)x) ++col;
    color[(size_t)x] = col;
    ncol = std::max(ncol, col + 1);
  }
  return ncol;
}

// Cuthill-McKee (deal.II) on the unconstrained cell-coupling graph of the DoF handler. Its nodes carry deal.II's
// per-support-point DoF groups: a velocity node's components followed by the pressure DoF at the same point
// (Q(k)-Q(kp) with kp | k: a pressure node sits on the velocity node of the same lexicographic position in every
// cell; the map is checked cell by cell). order[new index] = DoF.
int cuthill_mckee_order(const Layout &L, const IluPlanInput &in, std::vector<int64_t> &order, std::string &err) {
  const int dim = L.dim, nvc = L.nvc, npc = L.npc, ncn = L.ncn;
  const int64_t nv = L.nv, np = L.np, nc = L.nc, nu = L.nu, n = L.n;
  const bool sep = L.sep;
  std::vector<int64_t> p_at((size_t)std::max<int64_t>(np, 1), -1);  // pressure node -> velocity node
  bool p_map = sep && in.k % in.kp == 0;
  if (p_map) {
    const int r = in.k / in.kp, k1 = in.k + 1, kp1 = in.kp + 1;
    for (int64_t e = 0; e < nc && p_map; ++e)
      for (int a = 0; a < npc; ++a) {
        const int ax = a % kp1, ay = (a / kp1) % kp1, az = dim == 3 ? a / (kp1 * kp1) : 0;
        const int va = ax * r + k1 * (ay * r) + (dim == 3 ? k1 * k1 * az * r : 0);
        const int64_t pn = L.cp[(size_t)(e * npc + a)], vn = L.cv[(size_t)(e * nvc + va)];
        if (p_at[(size_t)pn] < 0) p_at[(size_t)pn] = vn;
        else if (p_at[(size_t)pn] != vn) { p_map = false; break; }
      }
  }
  // CM nodes: velocity nodes (+ their pressure DoF), then unmapped pressure nodes
  std::vector<int64_t> cmnode((size_t)nu, -1);  // unified node -> CM node
  int64_t ncm = 0;
  for (int64_t x = 0; x < nv; ++x) cmnode[(size_t)x] = ncm++;
  if (sep)
    for (int64_t pn = 0; pn < np; ++pn)  // (a ghost pressure node in no local cell -- a line master only -- is its own node)
      cmnode[(size_t)(nv + pn)] = p_map && p_at[(size_t)pn] >= 0 ? cmnode[(size_t)p_at[(size_t)pn]] : ncm++;
  std::vector<int64_t> cm_doff((size_t)ncm + 1, 0), cm_dofs((size_t)n);
  for (int64_t x = 0; x < nu; ++x) {
    int64_t d[4];
    int sl[4];
    cm_doff[(size_t)cmnode[(size_t)x] + 1] += L.node_dofs(x, d, sl);
  }
  for (int64_t y = 0; y < ncm; ++y) cm_doff[(size_t)y + 1] += cm_doff[(size_t)y];
  {
    std::vector<int64_t> f(cm_doff.begin(), cm_doff.end() - 1);
    for (int64_t x = 0; x < nu; ++x) {  // velocity nodes come first: their components precede p
      int64_t d[4];
      int sl[4];
      const int m = L.node_dofs(x, d, sl);
      for (int j = 0; j < m; ++j) cm_dofs[(size_t)f[(size_t)cmnode[(size_t)x]]++] = d[j];
    }
  }
  std::vector<int64_t> cadj_off((size_t)ncm + 1, 0), cadj;
  {
    std::vector<int64_t> ccoff((size_t)ncm + 1, 0), ccell;  // CM node -> cells
    for (int64_t e = 0; e < nc; ++e)
      for (int a = 0; a < ncn; ++a) ++ccoff[(size_t)cmnode[(size_t)L.cell_node(e, a)] + 1];
    for (int64_t y = 0; y < ncm; ++y) ccoff[(size_t)y + 1] += ccoff[(size_t)y];
    ccell.resize((size_t)ccoff[(size_t)ncm]);
    std::vector<int64_t> f(ccoff.begin(), ccoff.end() - 1);
    for (int64_t e = 0; e < nc; ++e)
      for (int a = 0; a < ncn; ++a) ccell[(size_t)f[(size_t)cmnode[(size_t)L.cell_node(e, a)]]++] = e;
    std::vector<int64_t> stamp((size_t)ncm, -1), buf;
    for (int64_t y = 0; y < ncm; ++y) {
      buf.clear();
      buf.push_back(y);
      stamp[(size_t)y] = y;
      for (int64_t t = ccoff[(size_t)y]; t < ccoff[(size_t)y + 1]; ++t)
        for (int a = 0; a < ncn; ++a) {
          const int64_t z = cmnode[(size_t)L.cell_node(ccell[(size_t)t], a)];
          if (stamp[(size_t)z] != y) { stamp[(size_t)z] = y; buf.push_back(z); }
        }
      std::sort(buf.begin(), buf.end());
      cadj.insert(cadj.end(), buf.begin(), buf.end());
      cadj_off[(size_t)y + 1] = (int64_t)cadj.size();
    }
  }
  cuthill_mckee_nodes(ncm, cadj_off, cadj, cm_doff, cm_dofs, order);
  if ((int64_t)order.size() != n)
    return fail(err, "gls_ilu_attach: renumbering covers %lld of %lld DoFs", (long long)order.size(), (long long)n);
  std::vector<char> seen((size_t)n, 0);
  for (int64_t d : order)
    if (d < 0 || d >= n || seen[(size_t)d]++) return fail(err, "gls_ilu_attach: renumbering is not a permutation");
  return 0;
}

// subdomains (Ifpack's additive Schwarz with overlap 0, which the reference runs with one block per MPI rank):
// contiguous ranges of the cell order (space-filling: leaf order of the forest / Morton bricks), a DoF in the block
// of its lowest cell; couplings between blocks are dropped, each block is factored on its own, the blocks'
// triangular solves run side by side
int assign_blocks(const Layout &L, int64_t block_dofs, const std::vector<int64_t> &dnode, std::vector<int32_t> &dblk) {
  const int64_t n = L.n, nc = L.nc;
  const int nblk = block_dofs > 0 ? (int)std::min<int64_t>(std::max<int64_t>((n + block_dofs - 1) / block_dofs, 1), nc) : 1;
  dblk.assign((size_t)n, 0);
  if (nblk > 1) {
    std::vector<int32_t> nodeblk((size_t)L.nu, INT32_MAX);
    for (int64_t e = 0; e < nc; ++e) {
      const int32_t b = (int32_t)(e * nblk / nc);
      for (int a = 0; a < L.ncn; ++a) {
        int32_t &nb_ = nodeblk[(size_t)L.cell_node(e, a)];
        nb_ = std::min(nb_, b);
      }
    }
    for (int64_t d = 0; d < n; ++d) {
      const int32_t b = nodeblk[(size_t)dnode[(size_t)d]];
      dblk[(size_t)d] = b == INT32_MAX ? 0 : b;
    }
  }
  return nblk;
}

// multicolor order: a greedy distance-1 coloring of the node graph of the system matrix (nodes visited in
// Cuthill-McKee order); DoFs sorted by (color, node's first Cuthill-McKee position, position), so a node's DoFs stay
// consecutive. Same-colored nodes share no matrix entry: each color's diagonal block is block-diagonal by node, and
// the triangular solves' dependency chain is ~colors x DoFs per node. (Blocks only drop couplings here: the colors
// stay outermost.) Returns the number of colours.
int multicolor_reorder(const IluCsr &graph, const std::vector<int64_t> &dnode, std::vector<int64_t> &order,
                       std::vector<int32_t> &dcolor) {
  const int64_t n = (int64_t)order.size(), nu = (int64_t)graph.off.size() - 1;
  // visit order of the greedy coloring: Cuthill-McKee (smallest-last ordering gave 36 instead of 46 colors but
  // 104 instead of 60 GMRES iterations, profiles/r03_ilu_coloring_ab.txt)
  std::vector<int64_t> visit, npos((size_t)nu, INT64_MAX), pos((size_t)n);
  visit.reserve((size_t)nu);
  for (int64_t t = 0; t < n; ++t) {
    pos[(size_t)order[(size_t)t]] = t;
    int64_t &np_ = npos[(size_t)dnode[(size_t)order[(size_t)t]]];
    if (np_ == INT64_MAX) {  // the node's first position
      np_ = t;
      visit.push_back(dnode[(size_t)order[(size_t)t]]);
    }
  }
  std::vector<int> c1;
  const int ncl = greedy_coloring(graph, visit.data(), 1, c1);
  dcolor.assign((size_t)n, 0);
  for (int64_t d = 0; d < n; ++d) dcolor[(size_t)d] = c1[(size_t)dnode[(size_t)d]];
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    if (dcolor[(size_t)a] != dcolor[(size_t)b]) return dcolor[(size_t)a] < dcolor[(size_t)b];
    const int64_t pa = npos[(size_t)dnode[(size_t)a]], pb = npos[(size_t)dnode[(size_t)b]];
    if (pa != pb) return pa < pb;
    return pos[(size_t)a] < pos[(size_t)b];
  });
  return ncl;
}

// complete owned rows: the system matrix's rows gain the neighbours' couplings; aown marks the entries probed on
// this rank
void merge_remote_entries(const std::vector<IluRemoteEntry> &remote, IluCsr &a, std::vector<char> &aown) {
  const int64_t n = (int64_t)a.off.size() - 1;
  std::vector<int64_t> xoff((size_t)n + 1, 0), extra(remote.size());  // row -> the records' columns, in record order
  for (const auto &r : remote) ++xoff[(size_t)r.i + 1];
  for (int64_t i = 0; i < n; ++i) xoff[(size_t)i + 1] += xoff[(size_t)i];
  {
    std::vector<int64_t> f(xoff.begin(), xoff.end() - 1);
    for (const auto &r : remote) extra[(size_t)f[(size_t)r.i]++] = r.j;
  }
  IluCsr m;
  m.off.assign((size_t)n + 1, 0);
  m.col.reserve(a.col.size() + extra.size());
  for (int64_t i = 0; i < n; ++i) {
    const size_t s0 = m.col.size();
    const auto b = a.col.begin() + a.off[(size_t)i], e = a.col.begin() + a.off[(size_t)i + 1];
    m.col.insert(m.col.end(), b, e);
    for (int64_t t = xoff[(size_t)i]; t < xoff[(size_t)i + 1]; ++t)
      if (!std::binary_search(b, e, extra[(size_t)t])) m.col.push_back(extra[(size_t)t]);
    std::sort(m.col.begin() + (std::ptrdiff_t)s0, m.col.end());
    m.col.erase(std::unique(m.col.begin() + (std::ptrdiff_t)s0, m.col.end()), m.col.end());
    m.off[(size_t)i + 1] = (int64_t)m.col.size();
  }
  aown.assign(m.col.size(), 0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t t = m.off[(size_t)i]; t < m.off[(size_t)i + 1]; ++t)
      aown[(size_t)t] = std::binary_search(a.col.begin() + a.off[(size_t)i], a.col.begin() + a.off[(size_t)i + 1], m.col[(size_t)t]);
  a.off.swap(m.off);
  a.col.swap(m.col);
}

// the system matrix's pattern in the new numbering (couplings between blocks dropped), each entry's ownership flag
void renumbered_pattern(const IluCsr &a, const std::vector<char> &aown, const std::vector<int32_t> &dblk,
                        const std::vector<int32_t> &newidx, const std::vector<int32_t> &olddof, std::vector<int64_t> &arow,
                        std::vector<int32_t> &acl, std::vector<char> &aclown) {
  const int64_t n = (int64_t)olddof.size();
  arow.assign((size_t)n + 1, 0);
  acl.clear();
  aclown.clear();
  acl.reserve(a.col.size());
  aclown.reserve(a.col.size());
  std::vector<std::pair<int32_t, char>> rowbuf;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t i = olddof[(size_t)r];
    rowbuf.clear();
    for (int64_t t = a.off[(size_t)i]; t < a.off[(size_t)i + 1]; ++t)
      if (dblk[(size_t)a.col[(size_t)t]] == dblk[(size_t)i]) rowbuf.push_back({newidx[(size_t)a.col[(size_t)t]], aown[(size_t)t]});
    std::sort(rowbuf.begin(), rowbuf.end());
    for (const auto &e : rowbuf) {
      acl.push_back(e.first);
      aclown.push_back(e.second);
    }
    arow[(size_t)r + 1] = (int64_t)acl.size();
  }
}

// multicolor solves: node groups (consecutive rows of one node), per color their range, per row the split of its
// entries into other colors / own node; valid while no entry couples two nodes of one color (fill 0; fill-in can
// create such entries: then P.mc_solve stays false)
void multicolor_groups(const std::vector<int32_t> &olddof, IluPlan &P) {
  const int64_t n = P.n;
  const int ncl = P.n_order_colors;
  const auto &rowp = P.rowp;
  const auto &col = P.col;
  const auto &dnode = P.dnode;
  const auto &dcolor = P.dcolor;
  std::vector<int32_t> cstart((size_t)ncl + 2, (int32_t)n), grow, cg((size_t)ncl + 1, 0);
  std::vector<int64_t> lsp((size_t)n), usp((size_t)n);
  for (int64_t r = n - 1; r >= 0; --r) cstart[(size_t)dcolor[(size_t)olddof[(size_t)r]]] = (int32_t)r;
  for (int c = ncl - 1; c >= 0; --c) cstart[(size_t)c] = std::min(cstart[(size_t)c], cstart[(size_t)c + 1]);
  bool ok = true;
  for (int64_t r = 0; r < n && ok; ++r) {
    const int64_t x = dnode[(size_t)olddof[(size_t)r]];
    if (r == 0 || x != dnode[(size_t)olddof[(size_t)r - 1]]) grow.push_back((int32_t)r);
    if (r + 1 - grow.back() > kPlanMaxGroupRows) ok = false;
    const int cr = dcolor[(size_t)olddof[(size_t)r]];
    int64_t e = rowp[(size_t)r];
    while (e < rowp[(size_t)r + 1] && col[(size_t)e] < cstart[(size_t)cr]) ++e;
    lsp[(size_t)r] = e;
    while (e < rowp[(size_t)r + 1] && col[(size_t)e] < cstart[(size_t)cr + 1]) {
      if (dnode[(size_t)olddof[(size_t)col[(size_t)e]]] != x) ok = false;  // same color, other node
      ++e;
    }
    usp[(size_t)r] = e;
  }
  if (!ok) return;
  grow.push_back((int32_t)n);
  for (int c = 0, g = 0; c <= ncl; ++c) {
    while (g + 1 < (int)grow.size() && grow[(size_t)g] < cstart[(size_t)c]) ++g;
    cg[(size_t)c] = c == ncl ? (int)grow.size() - 1 : g;
  }
  const size_t ng = grow.size() - 1;
  P.desc.assign(ng * kPlanGroupDesc, 0);
  for (size_t g = 0; g < ng; ++g) {
    int64_t *d = &P.desc[g * kPlanGroupDesc];
    const int32_t r0 = grow[g], nr = grow[g + 1] - r0;
    d[0] = r0;
    d[1] = nr;
    d[2] = rowp[(size_t)r0];
    d[3] = rowp[(size_t)(r0 + nr)];
    for (int t = 1; t < 4; ++t) d[3 + t] = t < nr ? rowp[(size_t)(r0 + t)] : INT64_MAX;
    for (int t = 0; t < nr; ++t) {
      d[8 + t] = lsp[(size_t)(r0 + t)];
      d[12 + t] = usp[(size_t)(r0 + t)];
      d[16 + t] = P.didx[(size_t)(r0 + t)];
      d[20 + t] = rowp[(size_t)(r0 + t) + 1];
    }
  }
  P.mc_solve = true;
  P.maxrow = 0;
  for (int64_t r = 0; r < n; ++r) P.maxrow = std::max(P.maxrow, rowp[(size_t)r + 1] - rowp[(size_t)r]);
  // the factorization's position map (uint16 per entry): per row, its first entry
  P.moff.assign((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; ++r) {
    int64_t m = 0;
    for (int64_t e = rowp[(size_t)r]; e < lsp[(size_t)r]; ++e) {
      const int32_t k = col[(size_t)e];
      m += (rowp[(size_t)k + 1] - P.didx[(size_t)k] - 1 + 3) & ~3;  // segments padded to quads
    }
    P.moff[(size_t)r + 1] = P.moff[(size_t)r] + m;
  }
  // per color and direction: one wavefront per node group while a group's other-color entries fit a few passes of
  // 64 lanes, else four (long rows: the late colors' L parts, the early colors' U parts)
  P.mc_wl.assign((size_t)ncl, 1);
  P.mc_wu.assign((size_t)ncl, 1);
  for (int c = 0; c < ncl; ++c) {
    const int32_t ra = grow[(size_t)cg[(size_t)c]], rb = grow[(size_t)cg[(size_t)c + 1]];
    const int ng_c = cg[(size_t)c + 1] - cg[(size_t)c];
    int64_t nlo = 0, nup = 0;
    for (int32_t r = ra; r < rb; ++r) {
      nlo += lsp[(size_t)r] - rowp[(size_t)r];
      nup += rowp[(size_t)r + 1] - usp[(size_t)r];
    }
    P.mc_wl[(size_t)c] = (uint8_t)(ng_c && nlo > 256 * (int64_t)ng_c ? 4 : 1);
    P.mc_wu[(size_t)c] = (uint8_t)(ng_c && nup > 256 * (int64_t)ng_c ? 4 : 1);
  }
  P.grow.swap(grow);
  P.cg.swap(cg);
  P.lsp.swap(lsp);
  P.usp.swap(usp);
}

// probes: one per (color, slot); every entry of the system matrix is read from the probe of its column DoF (entry
// position in the ILU pattern, row's original DoF). Ghost DoFs are not probed (identity rows): they are dropped from
// the unit lists, their diagonals remembered.
void probe_lists(const Layout &L, const std::vector<int64_t> &arow, const std::vector<int32_t> &acl,
                 const std::vector<char> &aclown, const std::vector<int32_t> &olddof, IluPlan &P) {
  const int64_t n = P.n;
  const int nprobe = P.n_probes;
  const auto &rowp = P.rowp;
  const auto &col = P.col;
  std::vector<int32_t> dprobe((size_t)n);
  for (int64_t d = 0; d < n; ++d) dprobe[(size_t)d] = P.probe_of(d);
  std::vector<int64_t> uoff((size_t)nprobe + 1, 0);
  P.peoff.assign((size_t)nprobe + 1, 0);
  // (complete rows: the unconstrained ghost DoFs are probed too)
  auto probed = [&](int64_t d) { return !L.ghost(d) || (P.complete && !P.fcons[(size_t)d]); };
  for (int64_t d = 0; d < n; ++d)
    if (probed(d)) ++uoff[(size_t)dprobe[(size_t)d] + 1];
  for (int64_t r = 0; r < n; ++r)
    for (int64_t t = arow[(size_t)r]; t < arow[(size_t)r + 1]; ++t)
      if (aclown[(size_t)t]) ++P.peoff[(size_t)dprobe[(size_t)olddof[(size_t)acl[(size_t)t]]] + 1];
  for (int p = 0; p < nprobe; ++p) {
    uoff[(size_t)p + 1] += uoff[(size_t)p];
    P.peoff[(size_t)p + 1] += P.peoff[(size_t)p];
  }
  P.pdofs.resize((size_t)uoff[(size_t)nprobe]);
  P.prow.resize((size_t)P.peoff[(size_t)nprobe]);
  P.pent.resize(P.prow.size());
  {
    std::vector<int64_t> f1(uoff.begin(), uoff.end() - 1), f2(P.peoff.begin(), P.peoff.end() - 1);
    for (int64_t d = 0; d < n; ++d)
      if (probed(d)) P.pdofs[(size_t)f1[(size_t)dprobe[(size_t)d]]++] = (int32_t)d;
    for (int64_t r = 0; r < n; ++r) {
      int64_t pos = rowp[(size_t)r];
      for (int64_t t = arow[(size_t)r]; t < arow[(size_t)r + 1]; ++t) {
        while (col[(size_t)pos] < acl[(size_t)t]) ++pos;  // both rows sorted; A's pattern is a subset
        if (!aclown[(size_t)t]) continue;
        const int64_t k = f2[(size_t)dprobe[(size_t)olddof[(size_t)acl[(size_t)t]]]]++;
        P.pent[(size_t)k] = pos;
        P.prow[(size_t)k] = olddof[(size_t)r];  // the probe result is indexed by the original DoF
      }
    }
  }
  P.pdoff.swap(uoff);
  P.ghost_diag.clear();
  for (int64_t r = 0; r < n; ++r)
    if (L.ghost(olddof[(size_t)r])) P.ghost_diag.push_back(P.didx[(size_t)r]);
  // probe of every unit DoF and every extracted entry (batched probing)
  P.pdpid.assign(std::max<size_t>(P.pdofs.size(), 1), 0);
  P.pepid.assign(std::max<size_t>(P.pent.size(), 1), 0);
  for (int p = 0; p < nprobe; ++p) {
    for (int64_t t = P.pdoff[(size_t)p]; t < P.pdoff[(size_t)p + 1]; ++t) P.pdpid[(size_t)t] = p;
    for (int64_t t = P.peoff[(size_t)p]; t < P.peoff[(size_t)p + 1]; ++t) P.pepid[(size_t)t] = p;
  }
}

// the neighbours' entries: per round, each CSR entry's send-list slots in (round, neighbour, slot) order
int remote_lists(const std::vector<IluRemoteEntry> &remote, const std::vector<int32_t> &dblk,
                 const std::vector<int32_t> &newidx, int n_rounds, IluPlan &P, std::string &err) {
  const auto &rowp = P.rowp;
  const auto &col = P.col;
  std::vector<std::pair<int64_t, int64_t>> key;  // (round * nnz + entry, record) sorted stably
  const int64_t nnz = (int64_t)col.size();
  for (size_t q = 0; q < remote.size(); ++q) {
    const auto &e = remote[q];
    if (dblk[(size_t)e.i] != dblk[(size_t)e.j]) continue;
    const int32_t r = newidx[(size_t)e.i], cj = newidx[(size_t)e.j];
    const auto b = col.begin() + rowp[(size_t)r], en = col.begin() + rowp[(size_t)r + 1];
    const auto it = std::lower_bound(b, en, cj);
    if (it == en || *it != cj) return fail(err, "gls_ilu_attach: a neighbour's entry is not in the pattern");
    key.push_back({(int64_t)e.round * nnz + (int64_t)(it - col.begin()), (int64_t)q});
  }
  std::stable_sort(key.begin(), key.end(), [](const std::pair<int64_t, int64_t> &a, const std::pair<int64_t, int64_t> &b) {
    return a.first < b.first;
  });
  P.ru.clear();
  P.ruoff.assign(1, 0);
  P.rslot.clear();
  P.rr.assign((size_t)std::max(n_rounds, 0) + 1, 0);
  for (size_t t = 0; t < key.size(); ++t) {
    if (t == 0 || key[t].first != key[t - 1].first) {
      if (t) P.ruoff.push_back((int32_t)P.rslot.size());
      P.ru.push_back(key[t].first % nnz);
      ++P.rr[(size_t)(key[t].first / nnz) + 1];
    }
    P.rslot.push_back(remote[(size_t)key[t].second].slot);
  }
  if (!key.empty()) P.ruoff.push_back((int32_t)P.rslot.size());
  for (int p = 0; p < n_rounds; ++p) P.rr[(size_t)p + 1] += P.rr[(size_t)p];
  P.ru.push_back(0);  // (padding: no zero-sized device buffers)
  P.rslot.push_back(0);
  P.n_rounds = n_rounds;
  return 0;
}

}  // namespace

int ilu_plan_patterns(const IluPlanInput &in, IluPlan &P, std::string &err) {
  if (in.dim < 2 || in.dim > 3 || in.k < 1 || in.kp < 1 || in.n_vnodes < 0 || in.n_pnodes < 0 || in.n_cells < 0)
    return fail(err, "gls_ilu_attach: plan input");
  const Layout L(in);
  const int64_t n = L.n, nu = L.nu;
  if ((int64_t)in.cell_vnodes.size() != L.nc * L.nvc || (L.sep && (int64_t)in.cell_pnodes.size() != L.nc * L.npc) ||
      (!L.sep && L.np != L.nv))
    return fail(err, "gls_ilu_attach: plan input");
  if (n >= INT32_MAX) return fail(err, "gls_ilu_attach: too many DoFs for 32-bit CSR");
  P = IluPlan();
  P.n = n;
  P.n_nodes = nu;
  P.slots = L.dim + 1;
  P.complete = L.dist;
  P.dnode.assign((size_t)n, 0);
  P.dslot.assign((size_t)n, 0);
  for (int64_t x = 0; x < nu; ++x) {
    int64_t d[4];
    int sl[4];
    const int m = L.node_dofs(x, d, sl);
    for (int j = 0; j < m; ++j) { P.dnode[(size_t)d[j]] = x; P.dslot[(size_t)d[j]] = sl[j]; }
  }
  // constrained DoFs (zero_constraints: Dirichlet + lines); the lines
  P.cons.assign((size_t)n, 0);
  for (int64_t d : in.con_dofs) P.cons[(size_t)d] = 1;
  std::vector<char> isline((size_t)n, 0);
  std::vector<int64_t> lidx((size_t)n, -1);
  for (size_t i = 0; i + 1 < in.h_off.size(); ++i) {
    lidx[(size_t)in.h_dof[i]] = (int64_t)i;
    isline[(size_t)in.h_dof[i]] = 1;
  }
  P.fcons = P.cons;  // constrained DoFs before the ghosts join them (complete rows)
  std::vector<char> dir((size_t)n);
  for (int64_t d = 0; d < n; ++d) {
    if (L.ghost(d)) P.cons[(size_t)d] = 1;
    dir[(size_t)d] = (P.cons[(size_t)d] && !isline[(size_t)d]) || L.ghost(d);
  }
  cell_pattern(L, in, lidx, P.cons, dir, P.a);
  node_graph(L, P.dnode, P.a, P.graph);
  // distance-2 coloring of the unified nodes in their natural order. Across ranks, complete owned rows (the rows of
  // Ifpack's distributed matrix, restricted to the owned columns as its additive Schwarz with overlap 0 does): the
  // owned x owned block also receives the neighbours' cells. Every rank probes its cells' operator on ALL its DoFs
  // (owned and ghost), so the coloring is that of the full local pattern's node graph.
  if (P.complete) {
    for (int64_t d = 0; d < n; ++d) dir[(size_t)d] = P.fcons[(size_t)d] && !isline[(size_t)d];
    cell_pattern(L, in, lidx, P.fcons, dir, P.fa);
    IluCsr fgraph;
    node_graph(L, P.dnode, P.fa, fgraph);
    P.n_probe_colors = greedy_coloring(fgraph, nullptr, 2, P.color);
  } else {
    P.n_probe_colors = greedy_coloring(P.graph, nullptr, 2, P.color);
  }
  P.n_probes = P.n_probe_colors * P.slots;
  return 0;
}

int ilu_plan_finish(const IluPlanInput &in, const std::vector<IluRemoteEntry> &remote, int n_rounds, IluPlan &P,
                    std::string &err) {
  const Layout L(in);
  const int64_t n = L.n;
  std::vector<char> aown;  // per system-matrix entry: probed on this rank (else a neighbour's entry only)
  if (P.complete) merge_remote_entries(remote, P.a, aown);
  else aown.assign(P.a.col.size(), 1);
  P.fa = IluCsr();  // the full pattern has served the tag exchange
  std::vector<int64_t> order;
  if (cuthill_mckee_order(L, in, order, err) != 0) return -1;
  std::vector<int32_t> dblk;
  P.n_blocks = assign_blocks(L, in.block_dofs, P.dnode, dblk);
  if (in.ordering == GLS_ILU_ORDER_MULTICOLOR)
    P.n_order_colors = multicolor_reorder(P.graph, P.dnode, order, P.dcolor);
  else if (P.n_blocks > 1)
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return dblk[(size_t)a] < dblk[(size_t)b]; });
  std::vector<int32_t> olddof((size_t)n);
  P.perm.assign((size_t)n, -1);
  for (int64_t r = 0; r < n; ++r) {
    P.perm[(size_t)order[(size_t)r]] = (int32_t)r;
    olddof[(size_t)r] = (int32_t)order[(size_t)r];
  }
  std::vector<int64_t> arow;
  std::vector<int32_t> acl;
  std::vector<char> aclown;
  renumbered_pattern(P.a, aown, dblk, P.perm, olddof, arow, acl, aclown);
  P.nnz_a = (int64_t)acl.size();
  if (iluk_pattern<int64_t>(n, arow.data(), acl.data(), in.fill, P.rowp, P.col) != GLS_OK)
    return fail(err, "gls_ilu_attach: ILU(%lld) pattern", in.fill);
  P.didx.assign((size_t)n, -1);
  for (int64_t r = 0; r < n; ++r) {
    const auto b = P.col.begin() + P.rowp[(size_t)r], e = P.col.begin() + P.rowp[(size_t)r + 1];
    const auto it = std::lower_bound(b, e, (int32_t)r);
    if (it == e || *it != r) return fail(err, "gls_ilu_attach: row %lld has no diagonal", (long long)r);
    P.didx[(size_t)r] = (int64_t)(it - P.col.begin());
  }
  if (in.ordering == GLS_ILU_ORDER_MULTICOLOR) multicolor_groups(olddof, P);
  probe_lists(L, arow, acl, aclown, olddof, P);
  return remote_lists(remote, dblk, P.perm, n_rounds, P, err);
}

}  // namespace gls

extern "C" int gls_ilu_plan(int dim, int k, int kp, int64_t n_vnodes, int64_t n_pnodes, int64_t n_cells,
                            const int32_t *cell_vnodes, const int32_t *cell_pnodes, int64_t n_con, const int64_t *con_dofs,
                            int64_t n_lines, const int64_t *line_dofs, const int64_t *line_offsets,
                            const int64_t *line_masters, int fill, int ordering, int64_t block_dofs, int32_t *perm,
                            int32_t *rowp, int32_t *col, int64_t capacity, int32_t *probe, int32_t *color,
                            int64_t *out_nnz, int64_t *out_nnz_a, int *out_n_probes, int *out_mc_solve) {
  if (!cell_vnodes || n_con < 0 || n_lines < 0 || (n_con > 0 && !con_dofs) ||
      (n_lines > 0 && (!line_dofs || !line_offsets || !line_masters)) || dim < 2 || dim > 3 || k < 1 || kp < 1 ||
      n_cells < 0)
    return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: bad arguments");
  if (fill < 0 || fill > GLS_ILU_MAX_FILL) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: fill out of range");
  if (ordering != GLS_ILU_ORDER_CM && ordering != GLS_ILU_ORDER_MULTICOLOR)
    return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: ordering");
  gls::IluPlanInput in;
  in.dim = dim, in.k = k, in.kp = kp;
  in.n_vnodes = n_vnodes, in.n_pnodes = n_pnodes, in.n_cells = n_cells;
  int nvc = 1, npc = 1;
  for (int i = 0; i < dim; ++i) nvc *= k + 1, npc *= kp + 1;
  in.cell_vnodes.assign(cell_vnodes, cell_vnodes + n_cells * nvc);
  if (cell_pnodes) in.cell_pnodes.assign(cell_pnodes, cell_pnodes + n_cells * npc);
  const int64_t n = (int64_t)dim * n_vnodes + n_pnodes;
  for (int64_t e = 0; e < n_cells * nvc; ++e)
    if (cell_vnodes[e] < 0 || cell_vnodes[e] >= n_vnodes) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: cell_vnodes");
  for (size_t e = 0; e < in.cell_pnodes.size(); ++e)
    if (cell_pnodes[e] < 0 || cell_pnodes[e] >= n_pnodes) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: cell_pnodes");
  in.con_dofs.assign(con_dofs, con_dofs + n_con);
  for (int64_t d : in.con_dofs)
    if (d < 0 || d >= n) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: constrained DoF out of range");
  if (n_lines > 0) {
    in.h_dof.assign(line_dofs, line_dofs + n_lines);
    in.h_off.assign(line_offsets, line_offsets + n_lines + 1);
    if (in.h_off[0] != 0) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: line offsets");
    for (int64_t i = 0; i < n_lines; ++i)
      if (in.h_off[(size_t)i + 1] < in.h_off[(size_t)i] || in.h_dof[(size_t)i] < 0 || in.h_dof[(size_t)i] >= n)
        return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: line");
    in.h_master.assign(line_masters, line_masters + in.h_off.back());
    for (int64_t m : in.h_master)
      if (m < 0 || m >= n) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: line master out of range");
  }
  in.fill = fill, in.ordering = ordering, in.block_dofs = block_dofs;
  gls::IluPlan P;
  std::string err;
  if (gls::ilu_plan_patterns(in, P, err) != 0 || gls::ilu_plan_finish(in, {}, 0, P, err) != 0)
    return gls_internal_set_err(GLS_EINVAL, err.c_str());
  const int64_t nnz = (int64_t)P.col.size();
  if (out_nnz) *out_nnz = nnz;
  if (out_nnz_a) *out_nnz_a = P.nnz_a;
  if (out_n_probes) *out_n_probes = P.n_probes;
  if (out_mc_solve) *out_mc_solve = P.mc_solve ? 1 : 0;
  if (!perm && !rowp && !col && !probe && !color) return GLS_OK;  // size query
  if (col && (capacity < nnz || nnz >= INT32_MAX)) return gls_internal_set_err(GLS_EINVAL, "gls_ilu_plan: capacity");
  for (int64_t d = 0; d < n; ++d) {
    if (perm) perm[d] = P.perm[(size_t)d];
    if (probe) probe[d] = P.probe_of(d);
    if (color) color[d] = P.dcolor.empty() ? -1 : P.dcolor[(size_t)d];
  }
  if (rowp)
    for (int64_t r = 0; r <= n; ++r) rowp[r] = (int32_t)P.rowp[(size_t)r];
  if (col) std::copy(P.col.begin(), P.col.end(), col);
  return GLS_OK;
}
