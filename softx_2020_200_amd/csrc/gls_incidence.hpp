// gls_incidence.hpp -- node -> (cell, slot) incidence of element vectors [n_cells][nv dim + np] (velocity slot a,
// component c at a * dim + c; pressure slot a at nv * dim + a), host only: for every velocity / pressure node the
// positions of its slots in ascending (cell, local node) order, the fixed summation order of
// gather_element_vectors. Shared by the per-cell operator path (ensure_element_maps) and the projection plan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gls_impl {

struct ElementIncidence {
  std::vector<int64_t> voff, vslot, poff, pslot;  // CSR: node n's slots are slot[off[n] .. off[n + 1])
};

// cv [n_cells][nv], cp [n_cells][np]: the cells' velocity / pressure nodes. false: a node id out of range
inline bool element_incidence(int64_t n_cells, int dim, int nv, int np, int64_t n_vnodes, int64_t n_pnodes,
                              const int32_t *cv, const int32_t *cp, ElementIncidence &I) {
  const int64_t el = (int64_t)nv * dim + np;
  for (int64_t e = 0; e < n_cells * nv; ++e)
    if (cv[e] < 0 || cv[e] >= n_vnodes) return false;
  for (int64_t e = 0; e < n_cells * np; ++e)
    if (cp[e] < 0 || cp[e] >= n_pnodes) return false;
  I.voff.assign((size_t)n_vnodes + 1, 0);
  I.poff.assign((size_t)n_pnodes + 1, 0);
  for (int64_t e = 0; e < n_cells * nv; ++e) ++I.voff[(size_t)cv[e] + 1];
  for (int64_t e = 0; e < n_cells * np; ++e) ++I.poff[(size_t)cp[e] + 1];
  for (size_t i = 1; i < I.voff.size(); ++i) I.voff[i] += I.voff[i - 1];
  for (size_t i = 1; i < I.poff.size(); ++i) I.poff[i] += I.poff[i - 1];
  I.vslot.assign((size_t)I.voff.back(), 0);
  I.pslot.assign((size_t)I.poff.back(), 0);
  std::vector<int64_t> vf(I.voff.begin(), I.voff.end() - 1), pf(I.poff.begin(), I.poff.end() - 1);
  for (int64_t cell = 0; cell < n_cells; ++cell) {
    for (int a = 0; a < nv; ++a) I.vslot[(size_t)vf[(size_t)cv[cell * nv + a]]++] = cell * el + (int64_t)a * dim;
    for (int a = 0; a < np; ++a) I.pslot[(size_t)pf[(size_t)cp[cell * np + a]]++] = cell * el + (int64_t)nv * dim + a;
  }
  return true;
}

}  // namespace gls_impl
