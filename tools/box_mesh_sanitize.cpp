// Stand-alone run of the subdivided hyper_rectangle's host-only code (csrc/gls_box_mesh.hpp: the mesh builder, the
// tile-Morton brick index and its inverse, the lattice check of build_slab_map) for the sanitizers: the tests' shapes
// and a few more with every mask, arrays sized exactly as gls_mesh_hyper_rectangle_sizes says (so a write past them is
// seen), index and inverse against each other over whole boxes, the lattice check accepting the open meshes and
// refusing periodic and perturbed ones, and the refusals. Exits 0 when all of it holds.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o box_mesh_sanitize
//       tools/box_mesh_sanitize.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../softx_2020_200_amd/csrc/gls_box_mesh.hpp"

static int fail(const char *what, long long a = 0, long long b = 0) {
  std::fprintf(stderr, "FAILED: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static int mesh_case(const int cells[3], int k, int kp, int mask) {
  int64_t nc = 0, nv = 0, np = 0;
  if (const char *why = gls_impl::box_mesh_sizes(cells, k, kp, mask, &nc, &nv, &np)) return fail(why);
  const int nvl = (k + 1) * (k + 1) * (k + 1), npl = (kp + 1) * (kp + 1) * (kp + 1);
  std::vector<int32_t> cv((size_t)(nc * nvl), -1), cp((size_t)(nc * npl), -1);
  std::vector<double> x0((size_t)(nc * 3)), h((size_t)(nc * 3));
  const double p1[3] = {0.0, -1.0, 0.5}, p2[3] = {2.0, 0.5, 3.5};
  if (const char *why = gls_impl::box_mesh_fill(cells, k, kp, p1, p2, mask, cv.data(), cp.data(), x0.data(), h.data()))
    return fail(why);
  std::vector<char> hit((size_t)nv, 0);
  for (int32_t v : cv) {
    if (v < 0 || v >= nv) return fail("velocity node out of range", v, nv);
    hit[(size_t)v] = 1;
  }
  for (char c : hit)
    if (!c) return fail("a velocity node in no cell");
  for (int32_t v : cp)
    if (v < 0 || v >= np) return fail("pressure node out of range", v, np);
  // the pressure arrays may be left out
  if (gls_impl::box_mesh_fill(cells, k, kp, p1, p2, mask, cv.data(), nullptr, nullptr, nullptr)) return fail("optional arrays");
  const int nb[3] = {cells[0] / 2, cells[1] / 2, cells[2] / 2};
  const int s = gls_impl::box_tile(nb);
  std::vector<char> seen((size_t)(nc / 8), 0);
  for (int bz = 0; bz < nb[2]; ++bz)
    for (int by = 0; by < nb[1]; ++by)
      for (int bx = 0; bx < nb[0]; ++bx) {
        const int64_t b = gls_impl::box_brick_index(nb, s, bx, by, bz);
        if (b < 0 || b >= nc / 8 || seen[(size_t)b]) return fail("brick index not a bijection", b, nc / 8);
        seen[(size_t)b] = 1;
        int bc[3];
        gls_impl::box_brick_coords(nb, s, b, bc);
        if (bc[0] != bx || bc[1] != by || bc[2] != bz) return fail("inverse of the brick index", b);
      }
  if (k <= 2) {
    int dnb[3] = {0, 0, 0}, ds = 0;
    const bool got = gls_impl::box_lattice_detect(nc, nv, k, cv.data(), dnb, &ds);
    if (got != (mask == 0)) return fail("lattice check", got, mask);
    if (got && (dnb[0] != nb[0] || dnb[1] != nb[1] || dnb[2] != nb[2] || ds != s)) return fail("lattice check counts");
    if (got && nc >= 16) {  // two cells exchanged, one node changed, a cell short: all refused
      std::vector<int32_t> w = cv;
      for (int a = 0; a < nvl; ++a) std::swap(w[(size_t)a], w[(size_t)((nc - 1) * nvl + a)]);
      if (gls_impl::box_lattice_detect(nc, nv, k, w.data(), dnb, &ds)) return fail("exchanged cells accepted");
      w = cv;
      w[w.size() - 1] -= 1;
      if (gls_impl::box_lattice_detect(nc, nv, k, w.data(), dnb, &ds)) return fail("changed node accepted");
      if (gls_impl::box_lattice_detect(nc - 8, nv, k, cv.data(), dnb, &ds)) return fail("short mesh accepted");
      if (gls_impl::box_lattice_detect(nc, nv - 1, k, cv.data(), dnb, &ds)) return fail("node count accepted");
    }
  }
  std::printf("cells %d x %d x %d k %d kp %d mask %d: %lld cells, %lld nodes, tiles of %d^3 bricks\n", cells[0], cells[1],
              cells[2], k, kp, mask, (long long)nc, (long long)nv, s);
  return 0;
}

int main() {
  const int shapes[][3] = {{2, 6, 4}, {4, 8, 12}, {8, 8, 4}, {4, 2, 6}, {2, 2, 2}, {4, 4, 4}, {8, 8, 8}, {16, 4, 8}, {12, 20, 4}};
  for (const auto &c : shapes)
    for (int k = 1; k <= 3; ++k)
      for (int mask = 0; mask < 8; ++mask)
        if (mesh_case(c, k, k == 2 ? (mask & 1 ? 1 : 2) : k, mask)) return 1;
  int64_t nc, nv, np;
  const int bad[][3] = {{3, 2, 2}, {2, 2, 5}, {0, 2, 2}, {2, -2, 2}, {2, 2, 1 << 21}, {1 << 12, 1 << 12, 1 << 12}};
  for (const auto &c : bad)
    if (!gls_impl::box_mesh_sizes(c, 1, 1, 0, &nc, &nv, &np)) return fail("not refused", c[0], c[2]);
  const int ok[3] = {2, 2, 2};
  if (!gls_impl::box_mesh_sizes(ok, 0, 1, 0, &nc, &nv, &np) || !gls_impl::box_mesh_sizes(ok, 1, 0, 0, &nc, &nv, &np) ||
      !gls_impl::box_mesh_sizes(ok, 1, 1, 8, &nc, &nv, &np) || !gls_impl::box_mesh_sizes(nullptr, 1, 1, 0, &nc, &nv, &np))
    return fail("bad arguments not refused");
  const double p[3] = {0, 0, 0};
  if (!gls_impl::box_mesh_fill(ok, 1, 1, p, p, 0, nullptr, nullptr, nullptr, nullptr)) return fail("null array not refused");
  int nb[3], s;
  if (gls_impl::box_lattice_detect(0, 0, 1, nullptr, nb, &s)) return fail("empty mesh accepted");
  std::printf("box mesh: ok\n");
  return 0;
}
