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

}  // namespace gls
