// HIP / CDNA4 (gfx950) kernels of the replicated coarse operator E at any dimE (coarse_dev.h): blocked Cholesky
// factorisation and blocked triangular sweeps.  Everything is stream-ordered on the library stream, has no host
// synchronisation, no inter-workgroup waiting and no floating-point atomics: the order between block steps is the
// stream's, every sum has one fixed order, and the same input gives the same bits on every run and every rank.
//
// Factorisation, right-looking, block size nb (E = L L^T, row-major, in place in L; L^T written as it is produced):
//   k_coarse_potrf_diag  the nb x nb diagonal block, ONE workgroup.  Column panels of 16: thread t holds row t of the
//                        panel in registers, pivots and the panel's top rows travel through LDS (two barriers per
//                        column); the finished panel is parked in LDS and the rest of the block is updated from it.
//   k_coarse_panel       the rows below: x L_kk^T = a by SUBSTITUTION, one thread per row (no inverted block: the
//                        componentwise bound |E - L L^T| <= gamma_{n+1} |L| |L^T| needs it), 16 columns in registers,
//                        L_kk read from the L^T copy (16 contiguous doubles, the same for every lane).
//   k_coarse_syrk        trailing update A -= P P^T, lower triangle only, v_mfma_f64_16x16x4_f64: a workgroup owns a
//                        64 x 64 block (four waves, 2 x 2 tiles of 16 x 16 each), P enters negated so that the MFMA
//                        accumulates A - P P^T in ascending k.
//   Operand maps of the f64 MFMA (k_mfma_selftest): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
//   C[row = (l >> 4) + 4 v][col = l & 15].
// A pivot with !(d > 0) sets the status word (first one wins) and the factorisation runs on over NaNs: no data-dependent
// control flow, so nothing can hang or leave its arrays.
//
// Sweeps, y <- (L L^T)^-1 y: per block row k_coarse_diag_solve (the scheme of k_chol_solve on nb unknowns, one workgroup)
// and k_coarse_gemv (the rows still to come minus their nb columns times the block just solved; one wave per row, lanes
// stride the columns, xor-butterfly sum: all fixed orders).  Forward with L below the block, backward with L^T above it.
//
// Sweeps on a block, Y <- (L L^T)^-1 Y with Y the n x w row-major slab (w = 16 | 32): the same two launches per block row,
// for all w columns together.  k_coarse_diag_solve_block is k_coarse_diag_solve with one workgroup per column (the same
// operations in the same order on Y[(k0 + t) w + j]); k_coarse_update_block is the matrix product of the rows still to
// come with the block just solved on v_mfma_f64_16x16x4_f64 -- one wave per 16-row tile, one or two 16-column tiles per
// wave, M enters negated and the accumulator starts at Y, so that it holds Y - M Y in ascending k.  An element of the
// result is one accumulation chain over its own column; the column's position, its neighbours and w do not enter.  Lanes
// outside the block (a ragged last row tile, kb no multiple of 4) feed exact zeros and store nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "backend.h"
#include "coarse_dev.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                 \
    }                                                                                      \
  } while (0)

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CF_IB = 16;      // columns of a register panel
constexpr int CF_MAXB = 256;   // largest block size (threads of the one-workgroup kernels)

// ------------------------------------------------------------------------------------------------ factorisation
__global__ __launch_bounds__(CF_MAXB) void k_coarse_potrf_diag(double* A, double* LT, int n, int k0, int kb, int* status) {
  __shared__ double s_pan[CF_MAXB][CF_IB + 1];
  __shared__ double s_col[2][CF_IB];
  __shared__ double s_piv[2];
  const int t = threadIdx.x;
  double* D = A + (int64_t)k0 * n + k0;
  for (int j0 = 0; j0 < kb; j0 += CF_IB) {
    const int jb = min(CF_IB, kb - j0);
    const bool mine = (t >= j0 && t < kb);
    double p[CF_IB];
#pragma unroll
    for (int c = 0; c < CF_IB; ++c) p[c] = (mine && c < jb) ? D[(int64_t)t * n + j0 + c] : 0.0;
#pragma unroll
    for (int c = 0; c < CF_IB; ++c) {
      if (c < jb) {                                   // (uniform)
        const int j = j0 + c;
        if (t == j) {
          const double d = p[c];
          if (!(d > 0.0) && *status == 0) *status = 1 + k0 + j;
          p[c] = sqrt(d);
          s_piv[c & 1] = p[c];
        }
        __syncthreads();
        if (mine && t > j) {
          p[c] = p[c] / s_piv[c & 1];
          if (t < j0 + jb) s_col[c & 1][t - j0] = p[c];
        }
        __syncthreads();
        if (mine && t > j) {
#pragma unroll
          for (int c2 = c + 1; c2 < CF_IB; ++c2)
            if (c2 < jb && t >= j0 + c2) p[c2] -= p[c] * s_col[c & 1][c2];
        }
      }
    }
    if (mine) {
#pragma unroll
      for (int c = 0; c < CF_IB; ++c) {
        if (c < jb && t >= j0 + c) {
          D[(int64_t)t * n + j0 + c] = p[c];
          LT[(int64_t)(k0 + j0 + c) * n + k0 + t] = p[c];
        }
        s_pan[t][c] = p[c];
      }
    }
    __syncthreads();
    const int w0 = j0 + jb, W = kb - w0;              // W > 0: jb == CF_IB
    for (int e = t; e < W * W; e += CF_MAXB) {
      const int r = w0 + e / W, cc = w0 + e % W;
      if (cc <= r) {
        double acc = D[(int64_t)r * n + cc];
#pragma unroll
        for (int c = 0; c < CF_IB; ++c) acc -= s_pan[r][c] * s_pan[cc][c];
        D[(int64_t)r * n + cc] = acc;
      }
    }
    __syncthreads();
  }
}

// rows r >= k0 + kb, columns k0 .. k0 + kb (kb a multiple of 16: a panel exists below full blocks only).  LTd: the L^T copy
// of the diagonal block (read), LTw: the same array (columns r of the rows k0 .. k0 + kb are written): disjoint elements.
__global__ __launch_bounds__(64) void k_coarse_panel(double* __restrict__ A, const double* __restrict__ LTd,
                                                     double* __restrict__ LTw, int n, int k0, int kb) {
  const int r = k0 + kb + blockIdx.x * 64 + threadIdx.x;
  if (r >= n) return;
  double* row = A + (int64_t)r * n + k0;
  for (int j0 = 0; j0 < kb; j0 += CF_IB) {
    double p[CF_IB];
#pragma unroll
    for (int c = 0; c < CF_IB; ++c) p[c] = row[j0 + c];
    for (int cp = 0; cp < j0; ++cp) {
      const double xv = row[cp];
      const double* lt = LTd + (int64_t)(k0 + cp) * n + k0 + j0;      // L_kk[j0 + c][cp], c = 0 .. 15
#pragma unroll
      for (int c = 0; c < CF_IB; ++c) p[c] -= xv * lt[c];
    }
#pragma unroll
    for (int c = 0; c < CF_IB; ++c) {
      const double* lt = LTd + (int64_t)(k0 + j0 + c) * n + k0 + j0;  // L_kk[j0 + c2][j0 + c]
      p[c] = p[c] / lt[c];
#pragma unroll
      for (int c2 = c + 1; c2 < CF_IB; ++c2) p[c2] -= p[c] * lt[c2];
    }
#pragma unroll
    for (int c = 0; c < CF_IB; ++c) {
      row[j0 + c] = p[c];
      LTw[(int64_t)(k0 + j0 + c) * n + r] = p[c];
    }
  }
}

// A[i][j] -= sum_k A[i][k0 + k] A[j][k0 + k], i >= j >= k0 + kb, k < kb (kb a multiple of 16)
__global__ __launch_bounds__(256) void k_coarse_syrk(double* A, int n, int k0, int kb) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int i0 = k0 + kb + bi * 64 + (w >> 1) * 32, j0 = k0 + kb + bj * 64 + (w & 1) * 32;
  if (i0 >= n || j0 >= n || j0 > i0 + 31) return;     // (wave-uniform) outside the matrix, or all above the diagonal
  const int li = l & 15, lk = l >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = i0 + 16 * a + lk + 4 * v, col = j0 + 16 * b + li;
        acc[a][b][v] = (row < n && col < n) ? A[(int64_t)row * n + col] : 0.0;
      }
  const double* ap[2];
  const double* bp[2];
  bool aok[2], bok[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int ra = i0 + 16 * a + li, rb = j0 + 16 * a + li;
    aok[a] = ra < n;
    bok[a] = rb < n;
    ap[a] = A + (int64_t)(aok[a] ? ra : 0) * n + k0 + lk;
    bp[a] = A + (int64_t)(bok[a] ? rb : 0) * n + k0 + lk;
  }
  for (int kk = 0; kk < kb; kk += 4) {
    double av[2], bv[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      av[a] = aok[a] ? -ap[a][kk] : 0.0;
      bv[a] = bok[a] ? bp[a][kk] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = i0 + 16 * a + lk + 4 * v, col = j0 + 16 * b + li;
        if (row < n && col <= row) A[(int64_t)row * n + col] = acc[a][b][v];
      }
}

__global__ __launch_bounds__(256) void k_coarse_zero_upper(double* L, int n) {
  const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c < n && c > r) L[(int64_t)r * n + c] = 0.0;
}

static bool block_ok(int nb) { return nb >= 16 && nb <= CF_MAXB && nb % 16 == 0; }

bool coarse_factor(const double* E, int n, int nb, double* L, double* LT, int* status) {
  if (!block_ok(nb)) throw std::runtime_error("coarse_factor: the block size must be a multiple of 16 in 16 .. 256");
  hipStream_t s = (hipStream_t)get_stream();
  HIPCHK(hipMemsetAsync(status, 0, sizeof(int), s));
  if (n <= 0) return true;
  const size_t bytes = sizeof(double) * (size_t)n * n;
  if (E != L) HIPCHK(hipMemcpyAsync(L, E, bytes, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(LT, 0, bytes, s));
  for (int k0 = 0; k0 < n; k0 += nb) {
    const int kb = std::min(nb, n - k0);
    hipLaunchKernelGGL(k_coarse_potrf_diag, dim3(1), dim3(CF_MAXB), 0, s, L, LT, n, k0, kb, status);
    const int m = n - k0 - kb;
    if (m > 0) {
      hipLaunchKernelGGL(k_coarse_panel, dim3((m + 63) / 64), dim3(64), 0, s, L, LT, LT, n, k0, kb);
      const int T = (m + 63) / 64;
      hipLaunchKernelGGL(k_coarse_syrk, dim3(T, T), dim3(256), 0, s, L, n, k0, kb);
    }
  }
  hipLaunchKernelGGL(k_coarse_zero_upper, dim3((n + 255) / 256, n), dim3(256), 0, s, L, n);
  HIPCHK(hipGetLastError());
  return true;
}

// ------------------------------------------------------------------------------------------------ sweeps
// The unknowns k0 .. k0 + kb of L z = y (forward) or L^T x = y (backward), in place; thread t owns unknown k0 + t.  Column
// k of the diagonal block of L is row k of L^T's (and vice versa): contiguous in t, PB of them in flight (k_chol_solve).
template <int PB>
__global__ __launch_bounds__(CF_MAXB) void k_coarse_diag_solve(const double* __restrict__ L, const double* __restrict__ LT,
                                                               int n, int k0, int kb, double* __restrict__ y, int backward) {
  __shared__ double xs[CF_MAXB];
  const int t = threadIdx.x;
  double yv = (t < kb) ? y[k0 + t] : 0.0;
  const double dg = (t < kb) ? L[(int64_t)(k0 + t) * n + k0 + t] : 1.0;
  if (!backward) {
    for (int q0 = 0; q0 < kb; q0 += PB) {
      double c[PB];
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = q0 + p;
        c[p] = (k < kb && t > k && t < kb) ? LT[(int64_t)(k0 + k) * n + k0 + t] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = q0 + p;
        if (k < kb) {                                   // (uniform)
          if (t == k) { yv = yv / dg; xs[k] = yv; }
          __syncthreads();
          if (t > k) yv -= c[p] * xs[k];
        }
      }
    }
  } else {
    for (int q0 = 0; q0 < kb; q0 += PB) {
      double c[PB];
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = kb - 1 - (q0 + p);
        c[p] = (k >= 0 && t < k) ? L[(int64_t)(k0 + k) * n + k0 + t] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = kb - 1 - (q0 + p);
        if (k >= 0) {
          if (t == k) { yv = yv / dg; xs[k] = yv; }
          __syncthreads();
          if (t < k) yv -= c[p] * xs[k];
        }
      }
    }
  }
  if (t < kb) y[k0 + t] = yv;
}

// y[r] -= sum_c M[r][k0 + c] y[k0 + c], c < kb, for the rows r0 <= r < r1 (none of them in the block); one wave per row
__global__ __launch_bounds__(256) void k_coarse_gemv(const double* __restrict__ M, int n, int k0, int kb, int r0, int r1,
                                                     double* y) {
  const int r = r0 + blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (r >= r1) return;                                  // (wave-uniform)
  const double* m = M + (int64_t)r * n + k0;
  double s = 0.0;
  for (int c = l; c < kb; c += 64) s += m[c] * y[k0 + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // a + b == b + a: every lane holds the same sum
  if (l == 0) y[r] -= s;
}

bool coarse_solve(const double* L, const double* LT, int n, int nb, double* y) {
  if (!block_ok(nb)) throw std::runtime_error("coarse_solve: the block size must be a multiple of 16 in 16 .. 256");
  if (n <= 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  for (int k0 = 0; k0 < n; k0 += nb) {                  // L z = y
    const int kb = std::min(nb, n - k0), th = ((kb + 63) / 64) * 64;
    hipLaunchKernelGGL((k_coarse_diag_solve<16>), dim3(1), dim3(th), 0, s, L, LT, n, k0, kb, y, 0);
    const int r0 = k0 + kb;
    if (r0 < n) hipLaunchKernelGGL(k_coarse_gemv, dim3((n - r0 + 3) / 4), dim3(256), 0, s, L, n, k0, kb, r0, n, y);
  }
  for (int k0 = ((n - 1) / nb) * nb; k0 >= 0; k0 -= nb) {   // L^T x = z, from the last block up
    const int kb = std::min(nb, n - k0), th = ((kb + 63) / 64) * 64;
    hipLaunchKernelGGL((k_coarse_diag_solve<16>), dim3(1), dim3(th), 0, s, L, LT, n, k0, kb, y, 1);
    if (k0 > 0) hipLaunchKernelGGL(k_coarse_gemv, dim3((k0 + 3) / 4), dim3(256), 0, s, LT, n, k0, kb, 0, k0, y);
  }
  HIPCHK(hipGetLastError());
  return true;
}

// ------------------------------------------------------------------------------------------------ sweeps on a block
// k_coarse_diag_solve on column j = blockIdx.x of the n x w row-major slab Y
template <int PB>
__global__ __launch_bounds__(CF_MAXB) void k_coarse_diag_solve_block(const double* __restrict__ L,
                                                                     const double* __restrict__ LT, int n, int k0, int kb,
                                                                     double* __restrict__ Y, int w, int backward) {
  __shared__ double xs[CF_MAXB];
  const int t = threadIdx.x;
  double* y = Y + (int64_t)k0 * w + blockIdx.x;
  double yv = (t < kb) ? y[(int64_t)t * w] : 0.0;
  const double dg = (t < kb) ? L[(int64_t)(k0 + t) * n + k0 + t] : 1.0;
  if (!backward) {
    for (int q0 = 0; q0 < kb; q0 += PB) {
      double c[PB];
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = q0 + p;
        c[p] = (k < kb && t > k && t < kb) ? LT[(int64_t)(k0 + k) * n + k0 + t] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = q0 + p;
        if (k < kb) {                                   // (uniform)
          if (t == k) { yv = yv / dg; xs[k] = yv; }
          __syncthreads();
          if (t > k) yv -= c[p] * xs[k];
        }
      }
    }
  } else {
    for (int q0 = 0; q0 < kb; q0 += PB) {
      double c[PB];
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = kb - 1 - (q0 + p);
        c[p] = (k >= 0 && t < k) ? L[(int64_t)(k0 + k) * n + k0 + t] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < PB; ++p) {
        const int k = kb - 1 - (q0 + p);
        if (k >= 0) {
          if (t == k) { yv = yv / dg; xs[k] = yv; }
          __syncthreads();
          if (t < k) yv -= c[p] * xs[k];
        }
      }
    }
  }
  if (t < kb) y[(int64_t)t * w] = yv;
}

// Y[r][:] -= sum_c M[r][k0 + c] Y[k0 + c][:], c < kb, for the rows r0 <= r < r1 (none of them in the block: the rows read
// and the rows written are disjoint, so the update is in place).  One wave per 16-row tile, CT column tiles of 16 (w = 16 CT).
template <int CT>
__global__ __launch_bounds__(256) void k_coarse_update_block(const double* __restrict__ M, int n, int k0, int kb, int r0,
                                                             int r1, double* Y) {
  constexpr int w = 16 * CT;
  const int l = threadIdx.x & 63, li = l & 15, lk = l >> 4;
  const int rt = r0 + (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (rt >= r1) return;                                 // (wave-uniform)
  d4 acc[CT];
#pragma unroll
  for (int b = 0; b < CT; ++b)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = rt + lk + 4 * v;
      acc[b][v] = (row < r1) ? Y[(int64_t)row * w + 16 * b + li] : 0.0;
    }
  // Operands: every lane loads from an address inside the block (row and k clamped) and lanes outside it take an exact
  // zero instead of what they loaded: the loads carry no predicate, so those of several k steps are in flight together.
  const bool aok = rt + li < r1;
  const double* ap = M + (int64_t)(aok ? rt + li : r0) * n + k0;
  const double* bp = Y + (int64_t)k0 * w + li;
  for (int k8 = 0; k8 < kb; k8 += 32) {                 // eight k steps' loads at a time
    double av[8], bv[8][CT];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k8 + 4 * u + lk;
      const bool kok = k < kb;
      const int kc = kok ? k : kb - 1;
      const double a = ap[kc];
      av[u] = (aok && kok) ? -a : 0.0;
#pragma unroll
      for (int b = 0; b < CT; ++b) {
        const double y = bp[(int64_t)kc * w + 16 * b];
        bv[u][b] = kok ? y : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k8 + 4 * u < kb) {                            // (uniform)
#pragma unroll
        for (int b = 0; b < CT; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u][b], acc[b], 0, 0, 0);
      }
  }
#pragma unroll
  for (int b = 0; b < CT; ++b)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = rt + lk + 4 * v;
      if (row < r1) Y[(int64_t)row * w + 16 * b + li] = acc[b][v];
    }
}

static void update_block(hipStream_t s, const double* M, int n, int k0, int kb, int r0, int r1, double* Y, int w) {
  const int wg = ((r1 - r0 + 15) / 16 + 3) / 4;
  if (w == 16) hipLaunchKernelGGL((k_coarse_update_block<1>), dim3(wg), dim3(256), 0, s, M, n, k0, kb, r0, r1, Y);
  else hipLaunchKernelGGL((k_coarse_update_block<2>), dim3(wg), dim3(256), 0, s, M, n, k0, kb, r0, r1, Y);
}

bool coarse_solve_block(const double* L, const double* LT, int n, int nb, double* Y, int w) {
  if (!block_ok(nb)) throw std::runtime_error("coarse_solve_block: the block size must be a multiple of 16 in 16 .. 256");
  if (w != 16 && w != 32) throw std::runtime_error("coarse_solve_block: width is not 16 or 32");
  if (n <= 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  for (int k0 = 0; k0 < n; k0 += nb) {                  // L Z = Y
    const int kb = std::min(nb, n - k0), th = ((kb + 63) / 64) * 64;
    hipLaunchKernelGGL((k_coarse_diag_solve_block<16>), dim3(w), dim3(th), 0, s, L, LT, n, k0, kb, Y, w, 0);
    if (k0 + kb < n) update_block(s, L, n, k0, kb, k0 + kb, n, Y, w);
  }
  for (int k0 = ((n - 1) / nb) * nb; k0 >= 0; k0 -= nb) {   // L^T X = Z, from the last block up
    const int kb = std::min(nb, n - k0), th = ((kb + 63) / 64) * 64;
    hipLaunchKernelGGL((k_coarse_diag_solve_block<16>), dim3(w), dim3(th), 0, s, L, LT, n, k0, kb, Y, w, 1);
    if (k0 > 0) update_block(s, LT, n, k0, kb, 0, k0, Y, w);
  }
  HIPCHK(hipGetLastError());
  return true;
}

}  // namespace bk
