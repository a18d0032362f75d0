// gls_vanka_maps.cpp -- host only: neighbour lists and overlap maps of the cell-Vanka patches (gls_vanka_maps.hpp) and
// their C export gls_vanka_maps.
#include "gls_vanka_maps.hpp"

#include <algorithm>

#include "../../include/gls_native.h"
#include "gls_error.hpp"

namespace gls {

namespace {
int ipow_i(int b, int e) { return e == 0 ? 1 : b * ipow_i(b, e - 1); }
}  // namespace

int build_vanka_maps(int dim, int k, int kp, int64_t n_cells, int64_t n_vnodes, int64_t n_pnodes, const int32_t *cv,
                     const int32_t *cp, VankaMaps &M, std::string &err) {
  M = VankaMaps();
  if (dim < 1 || dim > 3 || k < 1 || kp < 1 || kp > k || n_cells < 0 || n_vnodes < 0 || n_pnodes < 0 || (n_cells > 0 && !cv) ||
      (!cp && kp != k)) {
    err = "vanka maps: bad arguments";
    return -1;
  }
  const int nv = ipow_i(k + 1, dim), np = ipow_i(kp + 1, dim), nd = nv * dim + np;
  if (nd > 255) {
    err = "vanka maps: more than 255 DoFs per cell";
    return -1;
  }
  if (!cp) n_pnodes = n_vnodes;
  const int64_t n_dofs = (int64_t)dim * n_vnodes + n_pnodes;
  if (n_dofs >= INT32_MAX) {
    err = "vanka maps: DoF ids exceed 32 bits";
    return -1;
  }
  M.nd = nd;
  M.n_dofs = n_dofs;
  M.cell_dofs.resize((size_t)n_cells * nd);
  M.mult.assign((size_t)n_dofs, 0);
  for (int64_t c = 0; c < n_cells; ++c) {
    int32_t *d = M.cell_dofs.data() + c * nd;
    for (int a = 0; a < nv; ++a) {
      const int32_t n = cv[c * nv + a];
      if (n < 0 || n >= n_vnodes) {
        err = "vanka maps: velocity node out of range";
        return -1;
      }
      for (int e = 0; e < dim; ++e) d[a * dim + e] = n * dim + e;
    }
    for (int b = 0; b < np; ++b) {
      const int32_t n = cp ? cp[c * np + b] : cv[c * nv + b];
      if (n < 0 || n >= n_pnodes) {
        err = "vanka maps: pressure node out of range";
        return -1;
      }
      d[nv * dim + b] = (int32_t)((int64_t)dim * n_vnodes + n);
    }
    for (int i = 0; i < nd; ++i) ++M.mult[(size_t)d[i]];
  }
  // DoF -> cells, ascending
  std::vector<int64_t> doff((size_t)n_dofs + 1, 0);
  for (int64_t i = 0; i < n_dofs; ++i) doff[(size_t)i + 1] = doff[(size_t)i] + M.mult[(size_t)i];
  std::vector<int32_t> dcell((size_t)doff[(size_t)n_dofs]);
  {
    std::vector<int64_t> fill(doff.begin(), doff.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)
      for (int i = 0; i < nd; ++i) dcell[(size_t)fill[(size_t)M.cell_dofs[(size_t)(c * nd + i)]]++] = (int32_t)c;
  }
  std::vector<int32_t> pos((size_t)n_dofs, -1);  // local index in the current cell
  std::vector<int32_t> nb;
  M.nb_off.assign(1, 0);
  M.ov_off.assign(1, 0);
  for (int64_t c = 0; c < n_cells; ++c) {
    const int32_t *d = M.cell_dofs.data() + c * nd;
    for (int i = 0; i < nd; ++i) {
      if (pos[(size_t)d[i]] >= 0) {
        for (int j = 0; j < i; ++j) pos[(size_t)d[j]] = -1;
        err = "vanka maps: a cell holds a node twice (periodic identification)";
        return -1;
      }
      pos[(size_t)d[i]] = i;
    }
    nb.clear();
    for (int i = 0; i < nd; ++i)
      for (int64_t e = doff[(size_t)d[i]]; e < doff[(size_t)d[i] + 1]; ++e) nb.push_back(dcell[(size_t)e]);
    std::sort(nb.begin(), nb.end());
    nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
    for (int32_t c2 : nb) {
      const int32_t *d2 = M.cell_dofs.data() + (int64_t)c2 * nd;
      for (int j = 0; j < nd; ++j) {
        const int32_t i = pos[(size_t)d2[j]];
        if (i < 0) continue;
        M.ov_i.push_back((uint8_t)i);
        M.ov_j.push_back((uint8_t)j);
      }
      M.nb_cell.push_back(c2);
      M.ov_off.push_back((int64_t)M.ov_i.size());
    }
    M.nb_off.push_back((int64_t)M.nb_cell.size());
    for (int i = 0; i < nd; ++i) pos[(size_t)d[i]] = -1;
  }
  return 0;
}

}  // namespace gls

extern "C" int gls_vanka_maps(int dim, int k, int kp, int64_t n_cells, int64_t n_vnodes, int64_t n_pnodes,
                              const int32_t *cell_vnodes, const int32_t *cell_pnodes, int32_t *cell_dofs, int32_t *mult,
                              int64_t *nb_off, int32_t *nb_cell, int64_t nb_capacity, int64_t *ov_off, uint8_t *ov_i,
                              uint8_t *ov_j, int64_t ov_capacity, int64_t *out_pairs, int64_t *out_overlaps) {
  gls::VankaMaps M;
  std::string err;
  if (gls::build_vanka_maps(dim, k, kp, n_cells, n_vnodes, n_pnodes, cell_vnodes, cell_pnodes, M, err) != 0)
    return gls_internal_set_err(GLS_EINVAL, err.c_str());
  const int64_t npair = (int64_t)M.nb_cell.size(), nov = (int64_t)M.ov_i.size();
  if (out_pairs) *out_pairs = npair;
  if (out_overlaps) *out_overlaps = nov;
  if ((nb_cell || ov_off) && nb_capacity < npair) return gls_internal_set_err(GLS_EINVAL, "gls_vanka_maps: pair capacity");
  if ((ov_i || ov_j) && ov_capacity < nov) return gls_internal_set_err(GLS_EINVAL, "gls_vanka_maps: overlap capacity");
  if (cell_dofs) std::copy(M.cell_dofs.begin(), M.cell_dofs.end(), cell_dofs);
  if (mult) std::copy(M.mult.begin(), M.mult.end(), mult);
  if (nb_off) std::copy(M.nb_off.begin(), M.nb_off.end(), nb_off);
  if (nb_cell) std::copy(M.nb_cell.begin(), M.nb_cell.end(), nb_cell);
  if (ov_off) std::copy(M.ov_off.begin(), M.ov_off.end(), ov_off);
  if (ov_i) std::copy(M.ov_i.begin(), M.ov_i.end(), ov_i);
  if (ov_j) std::copy(M.ov_j.begin(), M.ov_j.end(), ov_j);
  return GLS_OK;
}
