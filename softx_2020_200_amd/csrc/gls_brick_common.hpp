// gls_brick_common.hpp — device helpers shared by the brick kernels (gls_brick_kernels.hip) and the
// pencil-dataflow J.v (gls_brick_pencil.hip).
#pragma once
#include "gls_common.hpp"

namespace gls {

// bijective XCD swizzle of n work items: orig % 8 labels the blocks that share an XCD (blocks b, b+8,
// ... land on one XCD); each XCD then walks a contiguous range of the items
__device__ __forceinline__ int xcd_swizzle(int orig, int n) {
  const int q = n / 8, r = n % 8, x = orig % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + orig / 8;
}

// rank of brick-lattice node (X, Y, Z) among the brick-boundary nodes (lexicographic, x fastest):
// its index minus the interior nodes that precede it
template <int BN>
__device__ __forceinline__ int bnd_index(int X, int Y, int Z) {
  constexpr int I = BN - 2;
  const int n = X + BN * (Y + BN * Z);
  int before = min(max(Z - 1, 0), I) * I * I;
  if (Z >= 1 && Z <= I) {
    before += min(max(Y - 1, 0), I) * I;
    if (Y >= 1 && Y <= I) before += min(max(X - 1, 0), I);
  }
  return n - before;
}

// every third bit of a Morton index: a brick's lattice coordinate (x: v, y: v >> 1, z: v >> 2)
__device__ __forceinline__ int morton_compact3(unsigned v) {
  v &= 0x09249249u;
  v = (v ^ (v >> 2)) & 0x030c30c3u;
  v = (v ^ (v >> 4)) & 0x0300f00fu;
  v = (v ^ (v >> 8)) & 0xff0000ffu;
  return (int)((v ^ (v >> 16)) & 0x3ffu);
}

// x / D for 0 <= x < N as one full-rate 24-bit multiply and a shift, (x * M) >> S: the compiler's division by a
// constant goes through v_mul_hi_u32 (quarter rate) and fix-up instructions, since it does not know the range.
// Exact for every x of the range: checked at compile time
template <unsigned D, unsigned M, unsigned S, unsigned N>
constexpr bool div_small_exact() {
  for (unsigned x = 0; x < N; ++x)
    if (((x * M) >> S) != x / D) return false;
  return true;
}
template <unsigned D, unsigned M, unsigned S, unsigned N>
__device__ __forceinline__ int div_small(int x) {
  static_assert(N <= (1u << 24) && M < (1u << 24) && (unsigned long long)N * M < (1ull << 32) && div_small_exact<D, M, S, N>(),
                "div_small: multiplier not exact on the range");
  return (int)(__umul24((unsigned)x, M) >> S);
}

// Node t (< 512) of a workgroup's up to 3 bricks of 5^3 nodes: brick bi = t / 125 and the node's lattice index
// n = X + 5 Y + 25 Z in the brick. A function of the thread index only: the gather and the epilogue of the pencil
// kernels both derive it here
struct BrickNodeIdx {
  int bi, n, X, Y, Z;
};
__device__ __forceinline__ BrickNodeIdx brick_node_idx(int t) {
  BrickNodeIdx r;
  r.bi = div_small<125, 525, 16, 512>(t);
  r.n = t - 125 * r.bi;
  r.Z = div_small<25, 164, 12, 128>(r.n);
  const int xy = r.n - 25 * r.Z;
  r.Y = div_small<5, 52, 8, 32>(xy);
  r.X = xy - 5 * r.Y;
  return r;
}

// a[bi] for a lane-varying bi in 0..2 and workgroup-uniform a[]: two selects on scalar operands
__device__ __forceinline__ int sel3(const int (&a)[3], int bi) { return bi == 0 ? a[0] : bi == 1 ? a[1] : a[2]; }

// Nested Q2 interpolation of a coarse cell onto the fine brick it contains, one line: the five fine values
// (local coordinate 0..4) from the line's three coarse values, rows 1 0 0 | 3/8 3/4 -1/8 | 0 1 0 | -1/8 3/4 3/8 | 0 0 1.
// Even coordinates copy their coarse value; odd ones lie inside this cell only and have one fixed term order. A
// node shared by several bricks therefore gets the same FP64 value from each of them when every brick applies
// this function along x, then y, then z: on the shared axis its coordinate is even (0 in one brick, 4 in the
// other), and both copy the same coarse line.
__device__ __forceinline__ void q2_prolong_line(double c0, double c1, double c2, double (&o)[5]) {
  o[0] = c0;
  o[1] = fma(-0.125, c2, fma(0.75, c1, 0.375 * c0));
  o[2] = c1;
  o[3] = fma(0.375, c2, fma(0.75, c1, -0.125 * c0));
  o[4] = c2;
}

// LDS hand-off between lanes of ONE wave: LDS ops of a wave execute in order; the asm keeps the
// compiler from moving LDS accesses across this point.
__device__ __forceinline__ void wave_sync() {
#ifdef GLS_WAVE_SYNC_DRAIN
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
  asm volatile("" ::: "memory");
#endif
  __builtin_amdgcn_wave_barrier();
}

// Q2 J.v linearization ("pencil" layout, 16 values per quadrature point): bricks are taken in triples
// (the pencil kernel's workgroup), a triple's 24 cells in 4 groups of 6 (one wave each), and per
// (triple, wave, qz, value) the 6 cells x 9 (qx, qy) points are 54 consecutive entries, lane
// 9 c + 3 qy + qx. A wave of the pencil kernel reads each (qz, value) as one contiguous 432-byte row.
constexpr int kQdpRow = 54;                       // entries per (triple, wave, qz, value) row
constexpr int kQdpTriple = 4 * 3 * kQData * kQdpRow;  // entries per brick triple (10368 = 3 x 3456)
__device__ __forceinline__ int64_t qdp_base(int brick, int ci, int q) {
  const int cw = (brick % 3) * 8 + ci, w = cw / 6, c = cw % 6;
  const int qx = q % 3, qy = (q / 3) % 3, qz = q / 9;
  return (int64_t)(brick / 3) * kQdpTriple + ((w * 3 + qz) * kQData) * kQdpRow + 9 * c + 3 * qy + qx;
}
// qdp_base(3 triple + b3, ci, qx + 3 qy) for a pencil lane (qz = 0), from the brick's triple and place in it (the
// pencil kernel holds them in scalar registers: no per-lane division of the brick index)
__device__ __forceinline__ int64_t qdp_base_lane(int triple, int b3, int ci, int qx, int qy) {
  const int cw = b3 * 8 + ci, w = div_small<6, 43, 8, 32>(cw), c = cw - 6 * w;
  return (int64_t)triple * kQdpTriple + (w * 3 * kQData) * kQdpRow + 9 * c + 3 * qy + qx;
}

}  // namespace gls
