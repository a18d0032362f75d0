// gls_vanka_maps.hpp -- host only: the mesh maps of the additive cell-Vanka smoother (gls_vanka_host.cpp). For every
// cell c its DoFs (the element-vector order: velocity node a, component d at a * dim + d, pressure node b at
// nv * dim + b), the cells c' that share a DoF with it in ascending order (c itself included), and per pair (c, c')
// the overlap: the local indices (i in c, j in c') of every shared DoF, ascending in j. The patch matrix is
//   A_c[i][i'] = sum over c' ascending of K_c'[j][j'] for the pairs (i, j), (i', j') of (c, c').
// No device code and no library state: tools/vanka_maps_sanitize.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace gls {

struct VankaMaps {
  int nd = 0;                     // DoFs per cell
  int64_t n_dofs = 0;
  std::vector<int32_t> cell_dofs; // [n_cells][nd]
  std::vector<int32_t> mult;      // [n_dofs] cells that hold the DoF
  std::vector<int64_t> nb_off;    // [n_cells + 1] -> nb_cell, ov_off
  std::vector<int32_t> nb_cell;   // neighbour cells of each cell, ascending
  std::vector<int64_t> ov_off;    // [n_pairs + 1] -> ov_i, ov_j
  std::vector<uint8_t> ov_i, ov_j;
};

// cv [n_cells][(k+1)^dim], cp [n_cells][(kp+1)^dim] (nullptr: the pressure sits on the velocity nodes, kp == k).
// 0, or -1 with err set: a node id out of range, more than 255 DoFs per cell, or a cell that holds a node twice
// (a periodic identification across one or two cells, which the cell patches do not cover)
int build_vanka_maps(int dim, int k, int kp, int64_t n_cells, int64_t n_vnodes, int64_t n_pnodes, const int32_t *cv,
                     const int32_t *cp, VankaMaps &M, std::string &err);

}  // namespace gls
