// The subdivided hyper_rectangle's mesh (gls_mesh_hyper_rectangle) and its brick order, host only: the builder, the
// closed form of the "tile-Morton" brick index that build_slab_map verifies and k_slab_sum_box evaluates, and the
// lattice check itself. No HIP, so that tools/box_mesh_sanitize.cpp runs all of it under the sanitizers.
//
// Order. cells[a] = 2 nb[a] cells per axis, bricks of 2 x 2 x 2 cells. s = the largest power of two dividing all
// three nb[a]; tiles of s^3 bricks run lexicographically (tx fastest), the bricks of a tile in Morton order of
// (bx % s, by % s, bz % s):
//   brick(bx, by, bz) = ((tz nty + ty) ntx + tx) s^3 + morton3(bx % s, by % s, bz % s),   t = b / s, nt = nb / s
// and the 8 cells of a brick in the order cx + 2 cy + 4 cz. On (n, n, n) with n a power of two this is the Morton
// order of gls_mesh_hyper_cube.
#pragma once
#include <cstdint>

namespace gls_impl {

inline int box_tile(const int nb[3]) {
  int s = 1;
  while (nb[0] % (2 * s) == 0 && nb[1] % (2 * s) == 0 && nb[2] % (2 * s) == 0) s *= 2;
  return s;
}

inline int64_t box_morton3(int64_t x, int64_t y, int64_t z) {
  int64_t m = 0;
  for (int b = 0; b < 21; ++b)
    m |= (((x >> b) & 1) << (3 * b)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b + 2));
  return m;
}

inline int64_t box_brick_index(const int nb[3], int s, int bx, int by, int bz) {
  const int64_t ntx = nb[0] / s, nty = nb[1] / s;
  const int64_t tile = ((int64_t)(bz / s) * nty + by / s) * ntx + bx / s;
  return tile * s * s * s + box_morton3(bx % s, by % s, bz % s);
}

// the inverse: brick b's coordinates
inline void box_brick_coords(const int nb[3], int s, int64_t b, int bc[3]) {
  const int64_t s3 = (int64_t)s * s * s, ntx = nb[0] / s, nty = nb[1] / s;
  const int64_t tile = b / s3, m = b % s3;
  int l[3] = {0, 0, 0};
  for (int bit = 0; bit < 21; ++bit)
    for (int a = 0; a < 3; ++a) l[a] |= (int)((m >> (3 * bit + a)) & 1) << bit;
  bc[0] = (int)(tile % ntx) * s + l[0];
  bc[1] = (int)((tile / ntx) % nty) * s + l[1];
  bc[2] = (int)(tile / (ntx * nty)) * s + l[2];
}

// nullptr, or what is wrong with the arguments
inline const char *box_mesh_sizes(const int cells[3], int k, int kp, int mask, int64_t *nc, int64_t *nv, int64_t *np) {
  if (!cells || k <= 0 || kp <= 0 || mask < 0 || mask > 7) return "hyper_rectangle: cells, k >= 1, kp >= 1, mask 0 - 7";
  int64_t c = 1, v = 1, p = 1;
  for (int a = 0; a < 3; ++a) {
    if (cells[a] < 2 || cells[a] % 2 != 0) return "hyper_rectangle: every cell count even and >= 2";
    if (cells[a] > (1 << 20)) return "hyper_rectangle: cell count too large";
    const bool per = (mask >> a) & 1;
    c *= cells[a];
    v *= (int64_t)k * cells[a] + (per ? 0 : 1);
    p *= (int64_t)kp * cells[a] + (per ? 0 : 1);
  }
  if (c > INT32_MAX || v > INT32_MAX || p > INT32_MAX) return "hyper_rectangle: too large for int32 ids";
  if (nc) *nc = c;
  if (nv) *nv = v;
  if (np) *np = p;
  return nullptr;
}

// cell's Qk nodes on the wrapped lexicographic lattice (x fastest): dm[a] = k cells[a] + (periodic ? 0 : 1)
inline void box_cell_nodes(const int ijk[3], int k, const int64_t dm[3], int32_t *out) {
  const int k1 = k + 1;
  for (int a = 0; a < k1 * k1 * k1; ++a) {
    const int loc[3] = {a % k1, (a / k1) % k1, a / (k1 * k1)};
    int64_t id = 0, stride = 1;
    for (int d = 0; d < 3; ++d) {
      id += (((int64_t)ijk[d] * k + loc[d]) % dm[d]) * stride;
      stride *= dm[d];
    }
    out[a] = (int32_t)id;
  }
}

inline const char *box_mesh_fill(const int cells[3], int k, int kp, const double p1[3], const double p2[3], int mask,
                                 int32_t *cv, int32_t *cp, double *x0, double *h) {
  int64_t nc = 0;
  if (const char *why = box_mesh_sizes(cells, k, kp, mask, &nc, nullptr, nullptr)) return why;
  if (!cv || !p1 || !p2) return "hyper_rectangle: null array";
  const int nb[3] = {cells[0] / 2, cells[1] / 2, cells[2] / 2};
  const int s = box_tile(nb);
  int64_t vd[3], pd[3];
  double hc[3];
  for (int a = 0; a < 3; ++a) {
    const bool per = (mask >> a) & 1;
    vd[a] = (int64_t)k * cells[a] + (per ? 0 : 1);
    pd[a] = (int64_t)kp * cells[a] + (per ? 0 : 1);
    hc[a] = (p2[a] - p1[a]) / cells[a];
  }
  const int nvl = (k + 1) * (k + 1) * (k + 1), npl = (kp + 1) * (kp + 1) * (kp + 1);
  for (int64_t b = 0; b < nc / 8; ++b) {
    int bc[3];
    box_brick_coords(nb, s, b, bc);
    for (int ci = 0; ci < 8; ++ci) {
      const int64_t cell = b * 8 + ci;
      const int ijk[3] = {2 * bc[0] + (ci & 1), 2 * bc[1] + ((ci >> 1) & 1), 2 * bc[2] + (ci >> 2)};
      box_cell_nodes(ijk, k, vd, cv + cell * nvl);
      if (cp) box_cell_nodes(ijk, kp, pd, cp + cell * npl);
      for (int d = 0; d < 3; ++d) {
        if (x0) x0[cell * 3 + d] = p1[d] + ijk[d] * hc[d];
        if (h) h[cell * 3 + d] = hc[d];
      }
    }
  }
  return nullptr;
}

// The open tile-Morton box, cell by cell: n_cells cells of (k+1)^3 nodes each against gls_mesh_hyper_rectangle's
// numbering with mask 0 for some nb[3] <= 2048 per axis. The counts are not in the mesh description; they follow
// from the cells themselves: on the open lexicographic lattice cell 0's node k+1 (local (0, 1, 0)) is NX, the last
// cell holds the last node, and the cell count gives the third. true: nb and s are set.
inline bool box_lattice_detect(int64_t n_cells, int64_t n_vnodes, int k, const int32_t *cv, int nb[3], int *s_out) {
  const int k1 = k + 1, n3 = k1 * k1 * k1;
  if (n_cells < 8 || n_cells % 8 != 0 || !cv) return false;
  const int64_t NX = cv[k1];  // node (0, 1, 0) of the cell at the origin
  if (cv[0] != 0 || NX < 2 * k + 1 || (NX - 1) % (2 * k) != 0) return false;
  const int64_t NXY = cv[k1 * k1];  // node (0, 0, 1): NX NY
  if (NXY < NX * (2 * k + 1) || NXY % NX != 0) return false;
  const int64_t NY = NXY / NX;
  if ((NY - 1) % (2 * k) != 0 || n_vnodes % NXY != 0) return false;
  const int64_t NZ = n_vnodes / NXY;
  if (NZ < 2 * k + 1 || (NZ - 1) % (2 * k) != 0) return false;
  const int64_t n[3] = {(NX - 1) / (2 * k), (NY - 1) / (2 * k), (NZ - 1) / (2 * k)};
  if (n[0] > 2048 || n[1] > 2048 || n[2] > 2048 || 8 * n[0] * n[1] * n[2] != n_cells) return false;
  const int nbb[3] = {(int)n[0], (int)n[1], (int)n[2]};
  const int s = box_tile(nbb);
  const int64_t dm[3] = {NX, NY, NZ};
  int32_t want[27];
  for (int64_t b = 0; b < n_cells / 8; ++b) {
    int bc[3];
    box_brick_coords(nbb, s, b, bc);
    for (int ci = 0; ci < 8; ++ci) {
      const int ijk[3] = {2 * bc[0] + (ci & 1), 2 * bc[1] + ((ci >> 1) & 1), 2 * bc[2] + (ci >> 2)};
      box_cell_nodes(ijk, k, dm, want);
      const int32_t *v = cv + (b * 8 + ci) * n3;
      for (int a = 0; a < n3; ++a)
        if (v[a] != want[a]) return false;
    }
  }
  for (int a = 0; a < 3; ++a) nb[a] = nbb[a];
  *s_out = s;
  return true;
}

}  // namespace gls_impl
