// Stand-alone run of the band-storage LU's host-only code (csrc/gls_band_layout.hpp: the layout and the bandwidth scan)
// for the sanitizers: the layouts the tests use and one past 2^31 floats, the refusals, and for small band matrices a
// host fill of the panels through the layout's offsets -- every entry lands inside its panel, no two share a float,
// and the panels read back as the matrix. Exits 0 when all of it holds.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o band_layout_sanitize
//       tools/band_layout_sanitize.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../softx_2020_200_amd/csrc/gls_band_layout.hpp"

using gls_impl::BandLayout;

static int fail(const char *what, long long a = 0, long long b = 0) {
  std::fprintf(stderr, "FAILED: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

// a band matrix as CSR, scanned and laid out; its entries written through at() into a 3 n nb array
static int fill_case(int64_t n, int64_t bl, int64_t bu, int64_t block) {
  std::vector<int64_t> rowp{0};
  std::vector<int32_t> col;
  for (int64_t r = 0; r < n; ++r) {
    for (int64_t c = r - bl < 0 ? 0 : r - bl; c <= r + bu && c < n; ++c) col.push_back((int32_t)c);
    rowp.push_back((int64_t)col.size());
  }
  int64_t sl = -1, su = -1;
  if (const char *why = gls_impl::csr_bandwidths(n, rowp.data(), col.data(), &sl, &su)) return fail(why);
  if (sl != (bl < n ? bl : n - 1) || su != (bu < n ? bu : n - 1)) return fail("bandwidth scan", sl, su);
  BandLayout L;
  if (const char *why = gls_impl::band_layout(n, sl, su, block, &L)) return fail(why);
  if (L.n_floats != 3 * n * L.nb || L.n_blocks != (n + L.nb - 1) / L.nb || L.nb % gls_impl::kBandSub) return fail("sizes");
  std::vector<float> P((size_t)L.n_floats, 0.f);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t e = rowp[(size_t)r]; e < rowp[(size_t)r + 1]; ++e) {
      const int64_t c = col[(size_t)e], at = L.at(r, c);
      if (at < L.panel(c / L.nb) || at >= L.panel(c / L.nb) + L.lda() * L.nb || at >= L.n_floats) return fail("outside its panel", r, c);
      if (P[(size_t)at] != 0.f) return fail("two entries share a float", r, c);
      P[(size_t)at] = (float)(1 + r * n + c);
    }
  // the blocks as the factorization addresses them: D_k at panel(k) + nb, U_k at panel(k + 1), lda = 3 nb
  for (int64_t k = 0; k < L.n_blocks; ++k)
    for (int64_t j = 0; j < L.nb && k * L.nb + j < n; ++j)
      for (int64_t i = 0; i < L.nb && k * L.nb + i < n; ++i) {
        const int64_t r = k * L.nb + i, c = k * L.nb + j;
        const bool in = r - c <= sl && c - r <= su;
        if (P[(size_t)(L.panel(k) + L.nb + j * L.lda() + i)] != (in ? (float)(1 + r * n + c) : 0.f)) return fail("D_k", r, c);
        if (k + 1 < L.n_blocks && c + L.nb < n) {
          const int64_t cu = c + L.nb;
          const bool inu = cu - r <= su;
          if (P[(size_t)(L.panel(k + 1) + j * L.lda() + i)] != (inu ? (float)(1 + r * n + cu) : 0.f)) return fail("U_k", r, cu);
        }
      }
  std::printf("n %lld bl %lld bu %lld block %lld -> nb %lld, %lld blocks, %lld floats\n", (long long)n, (long long)sl,
              (long long)su, (long long)block, (long long)L.nb, (long long)L.n_blocks, (long long)L.n_floats);
  return 0;
}

int main() {
  const int64_t shapes[][4] = {{1000, 100, 100, 128}, {777, 37, 200, 256}, {515, 0, 60, 128}, {515, 60, 0, 128},
                               {300, 250, 250, 256},  {100, 20, 20, 128},  {256, 30, 30, 128}, {700, 300, 290, 0},
                               {1, 0, 0, 0},          {129, 128, 128, 128}};
  for (const auto &s : shapes)
    if (fill_case(s[0], s[1], s[2], s[3])) return 1;
  BandLayout L;
  if (gls_impl::band_layout(400000, 8000, 8000, 0, &L) || L.nb != 8192 || L.n_blocks != 49 || L.n_floats != 9830400000LL)
    return fail("layout past 2^31", L.nb, L.n_floats);
  if (L.at(399999, 399999) >= L.n_floats || L.at(399999, 399999) < (int64_t)1 << 31) return fail("64-bit offset");
  const int64_t bad[][4] = {{0, 0, 0, 0},    {-5, 1, 1, 0},     {100, -1, 3, 0},   {100, 3, -1, 0},     {100, 3, 3, 64},
                            {100, 3, 3, 192}, {1000, 200, 3, 128}, {100, 100, 3, 0}, {INT32_MAX, 1, 1, 0}};
  for (const auto &b : bad)
    if (!gls_impl::band_layout(b[0], b[1], b[2], b[3], &L)) return fail("not refused", b[0], b[3]);
  int64_t bl = 0, bu = 0;
  const int64_t rp_bad[] = {0, 2, 1};
  const int32_t cl[] = {0, 1, 5};
  const int64_t rp[] = {0, 2, 3};
  if (!gls_impl::csr_bandwidths(2, rp_bad, cl, &bl, &bu) || !gls_impl::csr_bandwidths(2, rp, cl, &bl, &bu) ||
      !gls_impl::csr_bandwidths(0, rp, cl, &bl, &bu) || !gls_impl::csr_bandwidths(2, nullptr, cl, &bl, &bu))
    return fail("bad CSR not refused");
  std::printf("band layout: ok\n");
  return 0;
}
