// gls_lu_step.hpp -- internal, device code (included by gls_mg_kernels.hip and gls_band_lu.hip): the forward / backward
// substitution with an unpivoted FP32 LU factor (unit lower L below the diagonal, U on and above it), x overwritten,
// for the two storages of the coarsest level's factor. The scheme is one; the storages differ only in where entry
// (i, j) of a 128-wide sub-block column lies, which the kernel takes from an addressing policy:
//   LuDense: column-major n x n, lda = n (rocSOLVER getrf_npvt in place)
//   LuBand:  block-tridiagonal panels (gls_band_layout.hpp): column j starts at float j * 3 nb and holds the rows
//            (j / nb - 1) nb .. (j / nb + 2) nb - 1; a sub-block column never straddles two panels (128 | nb), so
//            inside one the panels read like a dense array with lda = 3 nb and a row shift nb - (j / nb) nb
// Block-column steps of kLuB rows: step k has the block k solution final; its workgroup 0 applies that block's column
// to the rows of the next block and solves the next diagonal block in LDS (one column at a time), the other workgroups
// apply it to the rows beyond. 2 n / kLuB launches per solve against rocBLAS trsv's 62 ms at n = 25000
// (profiles/r06_lu25k.txt).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace gls {
constexpr int kLuB = 128;
constexpr int kLuT = 256;

struct LuDense {
  int n;
  __device__ int64_t lda() const { return n; }
  __device__ int64_t shift(int) const { return 0; }  // added to a column's offset: the row origin of its storage
  __device__ int rmax(int) const { return n - 1; }   // the last row the column's storage holds
};
struct LuBand {
  int n, nb;
  __device__ int64_t lda() const { return 3 * (int64_t)nb; }
  __device__ int64_t shift(int cb) const { return nb - (int64_t)(cb / nb) * nb; }
  __device__ int rmax(int cb) const { return (int)min((int64_t)n, ((int64_t)(cb / nb) + 2) * nb) - 1; }
};

// Step k (k < 0: the first diagonal block alone, block 0 forward / the last block backward): workgroup 0 applies
// block column k to the next diagonal block's rows and solves that diagonal block, the others apply block column k
// to the rows beyond. A launch is bound by memory latency, so every global load of it is issued in ONE round before
// anything waits: the right-hand side, block k's solution, and the two 128 x 128 blocks workgroup 0 reads (its rows
// of block column k, the diagonal block), 16-byte loads along the columns, 16 + 16 per thread of 256, staged in LDS.
// (Rounds of dependent loads cost ~2 us each: 128 rounds of one load per thread, 72 / 113 us per forward / backward
// launch; rounds of 32, 21 us; profiles/r06_lu_solve_ab.txt.) The diagonal block is then solved by two wavefronts
// in turn, one column at a time with the column's value broadcast from its lane by v_readlane (no workgroup
// barrier in the sequential part; one hands the first half to the second).
template <bool LOWER, bool VEC, class Addr>
__global__ void __launch_bounds__(kLuT) k_lu_step(const float *__restrict__ A, Addr ad, float *__restrict__ x, int k,
                                                  int rlo) {  // rlo: backward, the first row block the others update
  __shared__ float xk[kLuB], xb[kLuB], rd[kLuB], part[2][kLuB];
  __shared__ float D[kLuB][kLuB + 1], C[kLuB][kLuB + 1];
  const int n = ad.n;
  const int t = threadIdx.x, nb = (n + kLuB - 1) / kLuB;
  const bool first = k < 0, diag = blockIdx.x == 0;
  const int j0 = first ? 0 : k * kLuB, nj = first ? 1 : min(kLuB, n - j0);
  const int kn = first ? (LOWER ? 0 : nb - 1) : (LOWER ? k + 1 : k - 1);  // the diagonal block solved here
  const int r0 = kn * kLuB, nr = min(kLuB, n - r0);
  const int rb = diag ? r0 : LOWER ? (k + 1 + (int)blockIdx.x) * kLuB : (rlo + (int)blockIdx.x - 1) * kLuB;  // row block
  const int row = t & (kLuB - 1), half = t >> 7;
  const int i = rb + row;
  const bool live = half == 0 && (diag ? row < nr : LOWER ? i < n : i < kn * kLuB);
  // the round of loads
  const float xi = x[min(i, n - 1)];
  const float xkt = first ? 0.f : x[j0 + min(row, nj - 1)];
  const int r4 = t & 31, cq = t >> 5;  // this thread's 4-row slot and column (of 8) in each 16-byte load round
  auto ld = [&](int rbase, int cb, int ncol, int q) {  // rows rbase.. of the columns cb.. (one sub-block column)
    const int rmax = ad.rmax(cb);
    const int r = rbase + 4 * r4;
    const int64_t c = (int64_t)(cb + min(q * 8 + cq, ncol - 1)) * ad.lda() + ad.shift(cb);
    if (VEC && r + 3 <= rmax) return *reinterpret_cast<const float4 *>(A + (c + r));
    return make_float4(A[c + min(r, rmax)], A[c + min(r + 1, rmax)], A[c + min(r + 2, rmax)], A[c + min(r + 3, rmax)]);
  };
  float4 qc[16], qd[16];
  if (!first) {
#pragma unroll
    for (int q = 0; q < 16; ++q) qc[q] = ld(rb, j0, nj, q);
  }
  if (diag) {
#pragma unroll
    for (int q = 0; q < 16; ++q) qd[q] = ld(r0, r0, nr, q);
  }
  if (half == 0) xk[row] = row < nj ? xkt : 0.f;
  if (!first) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = q * 8 + cq;
      C[4 * r4][c] = qc[q].x, C[4 * r4 + 1][c] = qc[q].y, C[4 * r4 + 2][c] = qc[q].z, C[4 * r4 + 3][c] = qc[q].w;
    }
  }
  if (diag) {  // outside the block: identity
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = q * 8 + cq;
      const float e[4] = {qd[q].x, qd[q].y, qd[q].z, qd[q].w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = 4 * r4 + u;
        D[rr][c] = rr < nr && c < nr ? e[u] : (rr == c ? 1.f : 0.f);
      }
    }
  }
  __syncthreads();
  float v = xi;
  if (!first) {  // the block column's product, two threads per row (halves of the columns)
    float sacc = 0.f;
#pragma unroll 16
    for (int c = 0; c < 64; ++c) sacc += C[row][64 * half + c] * xk[64 * half + c];  // (xk = 0 past the block)
    part[half][row] = sacc;
    __syncthreads();
    v = xi - part[0][row] - part[1][row];
  }
  if (!diag) {
    if (live) x[i] = v;
    return;
  }
  const int lane = t & 63, w = t >> 6;
  if (!LOWER && half == 0) {  // (read back by the writing wavefront only)
    rd[t] = 1.f / D[t][t];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  auto bcast = [](float q, int c) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q), c)); };
  auto tri = [&](int cb) {  // the wavefront's own 64 x 64 triangle
    if (LOWER) {
#pragma unroll
      for (int c = 0; c < 64; ++c) {
        const float xc = bcast(v, c), dv = D[t][cb + c];
        v = __builtin_fmaf(lane > c ? -dv : 0.f, xc, v);
      }
    } else {
      float xs = 0.f;
#pragma unroll
      for (int c = 63; c >= 0; --c) {
        const float xc = bcast(v, c) * rd[cb + c], dv = D[t][cb + c];
        xs = lane == c ? xc : xs;
        v = __builtin_fmaf(lane < c ? -dv : 0.f, xc, v);
      }
      v = xs;
    }
  };
  const int wf = LOWER ? 0 : 1;  // the wavefront solved first
  if (w == wf) {
    tri(64 * wf);
    xb[t] = v;
  }
  __syncthreads();
  if (w == 1 - wf) {
    const int cb = 64 * wf;
#pragma unroll 16
    for (int c = 0; c < 64; ++c) v -= D[t][cb + c] * xb[cb + c];
    tri(64 * w);
  }
  if (live) x[i] = v;
}

// the 2 ceil(n / kLuB) launches of one solve; bl / bu >= 0: lower / upper bandwidths -- a step updates only the row
// blocks its block column reaches (< 0: all of them)
template <bool VEC, class Addr>
void lu_solve_steps(const float *LU, Addr ad, float *x, hipStream_t s, int bl, int bu) {
  const int n = ad.n, nb = (n + kLuB - 1) / kLuB;
  hipLaunchKernelGGL((k_lu_step<true, VEC, Addr>), dim3(1), dim3(kLuT), 0, s, LU, ad, x, -1, 0);
  for (int k = 0; k + 1 < nb; ++k) {
    const int64_t end = bl < 0 ? n : std::min<int64_t>(n, (int64_t)(k + 1) * kLuB + bl);  // rows below reached by block column k
    const int64_t rest = end - (int64_t)(k + 2) * kLuB;
    hipLaunchKernelGGL((k_lu_step<true, VEC, Addr>), dim3(1 + (unsigned)(rest > 0 ? (rest + kLuB - 1) / kLuB : 0)),
                       dim3(kLuT), 0, s, LU, ad, x, k, 0);
  }
  hipLaunchKernelGGL((k_lu_step<false, VEC, Addr>), dim3(1), dim3(kLuT), 0, s, LU, ad, x, -1, 0);
  for (int k = nb - 1; k >= 1; --k) {
    const int rlo = bu < 0 ? 0 : (int)(std::max<int64_t>(0, (int64_t)k * kLuB - bu) / kLuB);  // rows above reached by block column k
    const int nblk = std::max(0, (k - 1) - rlo);
    hipLaunchKernelGGL((k_lu_step<false, VEC, Addr>), dim3(1 + nblk), dim3(kLuT), 0, s, LU, ad, x, k, rlo);
  }
}
}  // namespace gls
