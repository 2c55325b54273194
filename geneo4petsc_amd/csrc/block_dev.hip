// HIP / CDNA4 (gfx950) kernels of the block entry points (block_dev.h): slabs of w = 16 | 32 right-hand sides, row-major.
//
//   k_cheb_dir_block<FIRST, LAST, W>  the step of k_cheb_dir (cheb_dev.hip) on a slab.  One workgroup per chunk (at most
//                             1024 rows of ONE subdomain = one contiguous run of 1024 W doubles); (a, b) through scalar
//                             loads, pinned wave-uniform; 16-byte loads and stores (W is even, so both halves of a pair
//                             lie in one row and share its dscale); a stream of 40 B per entry, 48 B with out.
//   k_block_import / _export  column-major <-> slab through a 64-row LDS tile: the column-major side is walked along
//                             the rows, the slab side along its contiguous rows, both coalesced.
//   k_coldot1 / k_coldot2     per-column dot products: consecutive row ranges per workgroup (up to 1024 of them: four per
//                             CU), lanes own two columns (one 16-byte load per block) and every (512 / W)-th row, LDS
//                             reduction in index order, then one workgroup adds the partials in index order.  No atomics: the bits depend on n alone.
//   k_axpy_cols / k_xpby_cols per-column coefficients from a device array, 16-byte accesses.
//   k_chol_solve_block        k_chol_solve (backend_hip.hip) with one workgroup per column of Y.
// The elementwise kernels round every product and every sum (contraction off, as in cheb_dev.hip): the bits of the
// composed forms in core.cpp and of the numpy expressions in the tests.  The triangular sweeps keep the compiler's
// default contraction, which is what k_chol_solve is built with: the two must agree to the bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "block_dev.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                 \
    }                                                                                      \
  } while (0)

#pragma clang fp contract(off)

namespace bk {

typedef double blk_d2 __attribute__((ext_vector_type(2)));

static inline bool blk_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ double blk_uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

template <bool FIRST>
__device__ __forceinline__ void blk_cheb_step(double a, double b, double zv, double& dv, double& xv) {
  if (FIRST) {
    dv = __dmul_rn(a, zv);
    xv = dv;
  } else {
    dv = __dadd_rn(__dmul_rn(a, zv), __dmul_rn(b, dv));
    xv = __dadd_rn(xv, dv);
  }
}

// ---------------------------------------------------------------------------------------------- Chebyshev step
template <bool FIRST, bool LAST, int W>
__global__ __launch_bounds__(256) void k_cheb_dir_block(int nchunk, const int* __restrict__ start,
                                                        const int* __restrict__ len, const int* __restrict__ sub,
                                                        const double* __restrict__ coef, const double* Z, double* D,
                                                        double* X, const double* dscale, double* Out, int vec) {
  const int c = blockIdx.x;
  if (c >= nchunk) return;
  const int s = __builtin_amdgcn_readfirstlane(sub[c]);
  const int64_t r0 = start[c];
  const int ne = len[c] * W;                       // at most 1024 W entries
  const int64_t e0 = r0 * W;
  const double a = blk_uniform(coef[2 * (int64_t)s]);
  const double b = blk_uniform(coef[2 * (int64_t)s + 1]);
  const int t = threadIdx.x;
  if (!vec) {
    for (int e = t; e < ne; e += 256) {
      const int64_t i = e0 + e;
      double dv = 0.0, xv = 0.0;
      if (!FIRST) {
        dv = D[i];
        xv = X[i];
      }
      blk_cheb_step<FIRST>(a, b, Z[i], dv, xv);
      D[i] = dv;
      X[i] = xv;
      if (LAST) Out[i] = dscale ? __dmul_rn(dscale[r0 + e / W], xv) : xv;
    }
    return;
  }
  for (int p = t; p < (ne >> 1); p += 256) {       // W even: e0 and ne are even, entries 2 p and 2 p + 1 share a row
    const int64_t i = e0 + 2 * (int64_t)p;
    const blk_d2 zv = *reinterpret_cast<const blk_d2*>(Z + i);
    blk_d2 dv = {0.0, 0.0}, xv = {0.0, 0.0};
    if (!FIRST) {
      dv = *reinterpret_cast<const blk_d2*>(D + i);
      xv = *reinterpret_cast<const blk_d2*>(X + i);
    }
    double d0 = dv.x, d1 = dv.y, x0 = xv.x, x1 = xv.y;
    blk_cheb_step<FIRST>(a, b, zv.x, d0, x0);
    blk_cheb_step<FIRST>(a, b, zv.y, d1, x1);
    *reinterpret_cast<blk_d2*>(D + i) = blk_d2{d0, d1};
    *reinterpret_cast<blk_d2*>(X + i) = blk_d2{x0, x1};
    if (LAST) {
      if (dscale) {
        const double sv = dscale[r0 + (2 * p) / W];
        *reinterpret_cast<blk_d2*>(Out + i) = blk_d2{__dmul_rn(sv, x0), __dmul_rn(sv, x1)};
      } else {
        *reinterpret_cast<blk_d2*>(Out + i) = blk_d2{x0, x1};
      }
    }
  }
}

bool cheb_dir_block(const Chunks& c, const double* coef_k, int flags, const double* Z, double* D, double* X,
                    const double* dscale, double* Out, int w) {
  if (w != 16 && w != 32) throw std::runtime_error("cheb_dir_block: width is not 16 or 32");
  if (c.nchunk <= 0) return true;
  const bool first = (flags & 1) != 0, last = (flags & 2) != 0;
  if (!coef_k || !Z || !D || !X || (last && !Out)) throw std::runtime_error("cheb_dir_block: null argument");
  const int vec = blk_al16(Z) && blk_al16(D) && blk_al16(X) && (!last || blk_al16(Out)) ? 1 : 0;
  hipStream_t s = (hipStream_t)get_stream();
  const dim3 grid(c.nchunk), block(256);
#define BLK_LAUNCH(F, L, W_) \
  hipLaunchKernelGGL((k_cheb_dir_block<F, L, W_>), grid, block, 0, s, c.nchunk, c.start, c.len, c.sub, coef_k, Z, D, X, dscale, Out, vec)
#define BLK_FLAGS(W_)                            \
  do {                                           \
    if (first && last) BLK_LAUNCH(true, true, W_);   \
    else if (first) BLK_LAUNCH(true, false, W_);     \
    else if (last) BLK_LAUNCH(false, true, W_);      \
    else BLK_LAUNCH(false, false, W_);               \
  } while (0)
  if (w == 16) BLK_FLAGS(16);
  else BLK_FLAGS(32);
#undef BLK_FLAGS
#undef BLK_LAUNCH
  HIPCHK(hipGetLastError());
  return true;
}

// ---------------------------------------------------------------------------------------------- import / export
constexpr int BLK_TR = 64;      // rows of a tile; the LDS row stride BLK_TR + 1 keeps the transposed reads off one bank

template <int W>
__global__ __launch_bounds__(256) void k_block_import(const double* __restrict__ Xcm, int64_t ld, int n, int m,
                                                      double* __restrict__ Yrm) {
  __shared__ double tile[W][BLK_TR + 1];
  const int i0 = blockIdx.x * BLK_TR, t = threadIdx.x;
  const int rows = min(BLK_TR, n - i0);
  for (int e = t; e < m * BLK_TR; e += 256) {      // along the rows of one column: contiguous
    const int j = e / BLK_TR, i = e - j * BLK_TR;
    if (i < rows) tile[j][i] = Xcm[(int64_t)j * ld + i0 + i];
  }
  __syncthreads();
  for (int e = t; e < rows * W; e += 256) {        // along the slab's rows: contiguous
    const int i = e / W, j = e - i * W;
    Yrm[(int64_t)(i0 + i) * W + j] = (j < m) ? tile[j][i] : 0.0;
  }
}

template <int W>
__global__ __launch_bounds__(256) void k_block_export(const double* __restrict__ Xrm, int n, int m,
                                                      double* __restrict__ Ycm, int64_t ld) {
  __shared__ double tile[W][BLK_TR + 1];
  const int i0 = blockIdx.x * BLK_TR, t = threadIdx.x;
  const int rows = min(BLK_TR, n - i0);
  for (int e = t; e < rows * W; e += 256) {
    const int i = e / W, j = e - i * W;
    if (j < m) tile[j][i] = Xrm[(int64_t)(i0 + i) * W + j];
  }
  __syncthreads();
  for (int e = t; e < m * BLK_TR; e += 256) {
    const int j = e / BLK_TR, i = e - j * BLK_TR;
    if (i < rows) Ycm[(int64_t)j * ld + i0 + i] = tile[j][i];
  }
}

static void blk_check_shape(const char* what, int ld, int n, int m, int w) {
  if (w != 16 && w != 32) throw std::runtime_error(std::string(what) + ": width is not 16 or 32");
  if (m < 0 || m > w || n < 0 || ld < n) throw std::runtime_error(std::string(what) + ": bad shape");
}

bool block_import(const double* Xcm, int ld, int n, int m, double* Yrm, int w) {
  blk_check_shape("block_import", ld, n, m, w);
  if (n == 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const dim3 grid((n + BLK_TR - 1) / BLK_TR), block(256);
  if (w == 16) hipLaunchKernelGGL((k_block_import<16>), grid, block, 0, s, Xcm, (int64_t)ld, n, m, Yrm);
  else hipLaunchKernelGGL((k_block_import<32>), grid, block, 0, s, Xcm, (int64_t)ld, n, m, Yrm);
  HIPCHK(hipGetLastError());
  return true;
}

bool block_export(const double* Xrm, int w, int n, int m, double* Ycm, int ld) {
  blk_check_shape("block_export", ld, n, m, w);
  if (n == 0 || m == 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const dim3 grid((n + BLK_TR - 1) / BLK_TR), block(256);
  if (w == 16) hipLaunchKernelGGL((k_block_export<16>), grid, block, 0, s, Xrm, n, m, Ycm, (int64_t)ld);
  else hipLaunchKernelGGL((k_block_export<32>), grid, block, 0, s, Xrm, n, m, Ycm, (int64_t)ld);
  HIPCHK(hipGetLastError());
  return true;
}

// ---------------------------------------------------------------------------------------------- column dots
// VEC: 16-byte loads (both blocks 16-byte aligned); else the same lanes read the same two entries one by one: one order
template <int W, bool VEC>
__global__ __launch_bounds__(256) void k_coldot1(const double* __restrict__ X, const double* __restrict__ Y, int n,
                                                 int rows_per, double* __restrict__ work) {
  constexpr int H = W / 2;                         // a lane owns columns 2 c and 2 c + 1 ...
  constexpr int R = 256 / H;                       // ... of every R-th row of the workgroup's range
  __shared__ double red[R][W];
  const int t = threadIdx.x, c = t % H, rl = t / H;
  const int lo = blockIdx.x * rows_per, hi = min(n, lo + rows_per);
  double a0 = 0.0, a1 = 0.0;
  for (int i = lo + rl; i < hi; i += R) {
    const int64_t e = (int64_t)i * W + 2 * c;
    double x0, x1, y0, y1;
    if (VEC) {
      const blk_d2 xv = *reinterpret_cast<const blk_d2*>(X + e), yv = *reinterpret_cast<const blk_d2*>(Y + e);
      x0 = xv.x; x1 = xv.y; y0 = yv.x; y1 = yv.y;
    } else {
      x0 = X[e]; x1 = X[e + 1]; y0 = Y[e]; y1 = Y[e + 1];
    }
    a0 = __dadd_rn(a0, __dmul_rn(x0, y0));
    a1 = __dadd_rn(a1, __dmul_rn(x1, y1));
  }
  red[rl][2 * c] = a0;
  red[rl][2 * c + 1] = a1;
  __syncthreads();
  if (t < W) {
    double s = red[0][t];
    for (int r = 1; r < R; ++r) s = __dadd_rn(s, red[r][t]);
    work[(int64_t)blockIdx.x * W + t] = s;
  }
}

__global__ __launch_bounds__(64) void k_coldot2(const double* __restrict__ work, int nwg, int w, double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= w) return;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s = __dadd_rn(s, work[(int64_t)g * w + j]);
  out[j] = s;
}

bool block_coldot(const double* X, const double* Y, int n, int w, double* out, double* work) {
  if (w != 16 && w != 32) throw std::runtime_error("block_coldot: width is not 16 or 32");
  if (!out || !work || n < 0) throw std::runtime_error("block_coldot: bad argument");
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = std::max(1, std::min(BLOCK_COLDOT_WG, (n + 63) / 64));
  const int rows_per = (std::max(1, n) + nwg - 1) / nwg;
  const bool vec = blk_al16(X) && blk_al16(Y);
#define BLK_DOT(W_, V_) hipLaunchKernelGGL((k_coldot1<W_, V_>), dim3(nwg), dim3(256), 0, s, X, Y, n, rows_per, work)
  if (w == 16) { if (vec) BLK_DOT(16, true); else BLK_DOT(16, false); }
  else { if (vec) BLK_DOT(32, true); else BLK_DOT(32, false); }
#undef BLK_DOT
  hipLaunchKernelGGL(k_coldot2, dim3(1), dim3(64), 0, s, work, nwg, w, out);
  HIPCHK(hipGetLastError());
  return true;
}

// ---------------------------------------------------------------------------------------------- column updates
// XPBY false: Y = Y + c X (A = Y, B = X);  XPBY true: P = Z + c P (A = P, B = Z)
template <bool XPBY>
__device__ __forceinline__ double blk_colupd(double av, double bv, double cv) {
  return XPBY ? __dadd_rn(bv, __dmul_rn(cv, av)) : __dadd_rn(av, __dmul_rn(cv, bv));
}

template <bool XPBY>
__global__ __launch_bounds__(256) void k_cols(double* A, const double* B, const double* __restrict__ c, int64_t tot, int w,
                                              int vec) {
  const int64_t gs = (int64_t)gridDim.x * blockDim.x, g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vec) {
    for (int64_t e = g0; e < tot; e += gs) A[e] = blk_colupd<XPBY>(A[e], B[e], c[e & (w - 1)]);
    return;
  }
  for (int64_t p = g0; p < (tot >> 1); p += gs) {  // tot = n w is even; both entries lie in one row
    const int64_t e = 2 * p;
    const int j = (int)(e & (w - 1));
    const blk_d2 av = *reinterpret_cast<const blk_d2*>(A + e), bv = *reinterpret_cast<const blk_d2*>(B + e);
    *reinterpret_cast<blk_d2*>(A + e) = blk_d2{blk_colupd<XPBY>(av.x, bv.x, c[j]), blk_colupd<XPBY>(av.y, bv.y, c[j + 1])};
  }
}

template <bool XPBY>
static bool blk_cols(double* A, const double* B, const double* c, int n, int w, const char* what) {
  if (w != 16 && w != 32) throw std::runtime_error(std::string(what) + ": width is not 16 or 32");
  if (n <= 0) return true;
  if (!A || !B || !c) throw std::runtime_error(std::string(what) + ": null argument");
  const int64_t tot = (int64_t)n * w;
  const int vec = blk_al16(A) && blk_al16(B) ? 1 : 0;
  const int64_t work = vec ? tot / 2 : tot;
  const int grid = (int)std::min<int64_t>((work + 255) / 256, 8192);
  hipLaunchKernelGGL((k_cols<XPBY>), dim3(grid), dim3(256), 0, (hipStream_t)get_stream(), A, B, c, tot, w, vec);
  HIPCHK(hipGetLastError());
  return true;
}
bool block_axpy_cols(double* Y, const double* X, const double* c, int n, int w) {
  return blk_cols<false>(Y, X, c, n, w, "block_axpy_cols");
}
bool block_xpby_cols(double* P, const double* Z, const double* c, int n, int w) {
  return blk_cols<true>(P, Z, c, n, w, "block_xpby_cols");
}

// ---------------------------------------------------------------------------------------------- coarse solve, w columns
// k_chol_solve of backend_hip.hip, statement for statement, on column blockIdx.x of Y (stride w): thread t owns unknown t
// of that column; the compiler's default contraction, as there.
#pragma clang fp contract(fast)
template <int PB>
__global__ __launch_bounds__(1024) void k_chol_solve_block(const double* __restrict__ L, const double* __restrict__ LT,
                                                           int n, double* __restrict__ Y, int w) {
  extern __shared__ double xs[];   // n published unknowns
  const int t = threadIdx.x;
  double* y = Y + blockIdx.x;
  double yv = (t < n) ? y[(int64_t)t * w] : 0.0;
  const double dg = (t < n) ? L[(int64_t)t * n + t] : 1.0;
  for (int k0 = 0; k0 < n; k0 += PB) {                 // L z = b
    double c[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int k = k0 + p;
      c[p] = (k < n && t > k && t < n) ? LT[(int64_t)k * n + t] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int k = k0 + p;
      if (k < n) {                                     // (uniform)
        if (t == k) { yv = yv / dg; xs[k] = yv; }
        __syncthreads();
        if (t > k) yv -= c[p] * xs[k];
      }
    }
  }
  for (int k0 = 0; k0 < n; k0 += PB) {                 // L^T x = z, from the last unknown down
    double c[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int k = n - 1 - (k0 + p);
      c[p] = (k >= 0 && t < k) ? L[(int64_t)k * n + t] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int k = n - 1 - (k0 + p);
      if (k >= 0) {
        if (t == k) { yv = yv / dg; xs[k] = yv; }
        __syncthreads();
        if (t < k) yv -= c[p] * xs[k];
      }
    }
  }
  if (t < n) y[(int64_t)t * w] = yv;
}
#pragma clang fp contract(off)

bool chol_solve_block(const double* L, const double* LT, int n, double* Y, int w) {
  if (w != 16 && w != 32) throw std::runtime_error("chol_solve_block: width is not 16 or 32");
  if (n <= 0) return true;
  if (n > 1024) return false;
  const int threads = ((n + 63) / 64) * 64;
  hipLaunchKernelGGL((k_chol_solve_block<16>), dim3(w), dim3(threads), sizeof(double) * n, (hipStream_t)get_stream(), L, LT,
                     n, Y, w);
  HIPCHK(hipGetLastError());
  return true;
}

}  // namespace bk
