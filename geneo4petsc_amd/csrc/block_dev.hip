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
//   k_gs_dots1 / k_gs_dots2   the Gram-Schmidt coefficients of a block GMRES step: k_coldot1 / k_coldot2 for up to BLOCK_GS_GROUP
//                             left factors per pass over the right one (slab pointers from a device table), same bits per slab.
//   k_gs_update               y <- y + sum_i c_i .* v_i in one pass, i in order, one rounded product and sum each (the bits of
//                             successive k_axpy_cols), on k_coldot1's row ranges and lanes so that the squares of the result
//                             can be summed in its order; k_scale_cols: out = c .* x.
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

// ---------------------------------------------------------------------------------------------- Gram-Schmidt on slabs
// k_gs_dots1 is k_coldot1 with up to BLOCK_GS_GROUP left factors per pass over W: workgroup blockIdx.x takes the row range
// k_coldot1 gives it, lane t the rows and the two columns k_coldot1 gives it, and every slab of the group (blockIdx.y) has
// its own pair of accumulators, fed in row order with rounded products and sums: slab by slab the arithmetic of k_coldot1,
// so the partials, and with k_gs_dots2 (= k_coldot2 per slab) the sums, have its bits.  The slab pointers come from a
// device table; whether all of them allow 16-byte loads is decided here, once per workgroup (wave-uniform).
template <int W, bool VEC>
__device__ __forceinline__ void gs_dots_rows(const double* const (&vp)[BLOCK_GS_GROUP], int ng, const double* Wm, int lo,
                                             int hi, int c, int rl, double (&a0)[BLOCK_GS_GROUP],
                                             double (&a1)[BLOCK_GS_GROUP]) {
  constexpr int R = 256 / (W / 2);
  for (int i = lo + rl; i < hi; i += R) {
    const int64_t e = (int64_t)i * W + 2 * c;
    double w0, w1;
    if (VEC) {
      const blk_d2 wv = *reinterpret_cast<const blk_d2*>(Wm + e);
      w0 = wv.x; w1 = wv.y;
    } else {
      w0 = Wm[e]; w1 = Wm[e + 1];
    }
#pragma unroll
    for (int g = 0; g < BLOCK_GS_GROUP; ++g) {
      if (g < ng) {                                  // (uniform)
        double x0, x1;
        if (VEC) {
          const blk_d2 xv = *reinterpret_cast<const blk_d2*>(vp[g] + e);
          x0 = xv.x; x1 = xv.y;
        } else {
          x0 = vp[g][e]; x1 = vp[g][e + 1];
        }
        a0[g] = __dadd_rn(a0[g], __dmul_rn(x0, w0));
        a1[g] = __dadd_rn(a1[g], __dmul_rn(x1, w1));
      }
    }
  }
}

template <int W>
__global__ __launch_bounds__(256) void k_gs_dots1(const double* const* __restrict__ V, int nb, const double* __restrict__ Wm,
                                                  int n, int rows_per, double* __restrict__ work) {
  constexpr int H = W / 2, R = 256 / H, G = BLOCK_GS_GROUP;
  __shared__ double red[G][R][W];
  const int t = threadIdx.x, c = t % H, rl = t / H;
  const int lo = blockIdx.x * rows_per, hi = min(n, lo + rows_per);
  const int i0 = blockIdx.y * G, ng = min(G, nb - i0);
  const double* vp[G];
  uintptr_t bits = reinterpret_cast<uintptr_t>(Wm);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    vp[g] = V[i0 + min(g, ng - 1)];
    bits |= reinterpret_cast<uintptr_t>(vp[g]);
  }
  double a0[G], a1[G];
#pragma unroll
  for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0;
  if ((bits & 15u) == 0) gs_dots_rows<W, true>(vp, ng, Wm, lo, hi, c, rl, a0, a1);
  else gs_dots_rows<W, false>(vp, ng, Wm, lo, hi, c, rl, a0, a1);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    red[g][rl][2 * c] = a0[g];
    red[g][rl][2 * c + 1] = a1[g];
  }
  __syncthreads();
  for (int e = t; e < ng * W; e += 256) {
    const int g = e / W, j = e - g * W;
    double s = red[g][0][j];
    for (int r = 1; r < R; ++r) s = __dadd_rn(s, red[g][r][j]);
    work[((int64_t)(i0 + g) * gridDim.x + blockIdx.x) * W + j] = s;
  }
}

__global__ __launch_bounds__(64) void k_gs_dots2(const double* __restrict__ work, int nwg, int w, double* __restrict__ H) {
  const int j = threadIdx.x, i = blockIdx.x;
  if (j >= w) return;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s = __dadd_rn(s, work[((int64_t)i * nwg + g) * w + j]);
  H[(int64_t)i * w + j] = s;
}

bool block_gs_dots(const double* const* V, int nb, const double* Wm, int n, int w, double* H, double* work) {
  if (w != 16 && w != 32) throw std::runtime_error("block_gs_dots: width is not 16 or 32");
  if (nb < 0 || n < 0 || (nb > 0 && (!V || !Wm || !H || !work))) throw std::runtime_error("block_gs_dots: bad argument");
  if (nb == 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = block_coldot_nwg(n), rows_per = block_coldot_rows_per(n);
  const dim3 grid(nwg, (nb + BLOCK_GS_GROUP - 1) / BLOCK_GS_GROUP);
  if (w == 16) hipLaunchKernelGGL((k_gs_dots1<16>), grid, dim3(256), 0, s, V, nb, Wm, n, rows_per, work);
  else hipLaunchKernelGGL((k_gs_dots1<32>), grid, dim3(256), 0, s, V, nb, Wm, n, rows_per, work);
  hipLaunchKernelGGL(k_gs_dots2, dim3(nb), dim3(64), 0, s, work, nwg, w, H);
  HIPCHK(hipGetLastError());
  return true;
}

// k_gs_update: y <- fl(y + fl(c_i v_i)), i = 0 .. nb - 1 in that order, on the entries a lane of k_coldot1 owns, so that
// the squares of the result can be summed in its order (NORM): the partials of block_coldot(Y', Y').  The coefficients of
// a launch (at most BLK_GS_NBMAX slabs; the wrapper splits longer lists) sit in LDS.
constexpr int BLK_GS_NBMAX = 64;

template <int W, bool NORM, bool VEC>
__device__ __forceinline__ void gs_update_rows(double* Y, const double* const* __restrict__ V, int nb, const double* cs, int lo,
                                               int hi, int c, int rl, double& a0, double& a1) {
  constexpr int R = 256 / (W / 2);
  for (int i = lo + rl; i < hi; i += R) {
    const int64_t e = (int64_t)i * W + 2 * c;
    double y0, y1;
    if (VEC) {
      const blk_d2 yv = *reinterpret_cast<const blk_d2*>(Y + e);
      y0 = yv.x; y1 = yv.y;
    } else {
      y0 = Y[e]; y1 = Y[e + 1];
    }
#pragma unroll 4
    for (int k = 0; k < nb; ++k) {
      const double* v = V[k];
      double x0, x1;
      if (VEC) {
        const blk_d2 xv = *reinterpret_cast<const blk_d2*>(v + e);
        x0 = xv.x; x1 = xv.y;
      } else {
        x0 = v[e]; x1 = v[e + 1];
      }
      y0 = __dadd_rn(y0, __dmul_rn(cs[k * W + 2 * c], x0));
      y1 = __dadd_rn(y1, __dmul_rn(cs[k * W + 2 * c + 1], x1));
    }
    if (VEC) {
      *reinterpret_cast<blk_d2*>(Y + e) = blk_d2{y0, y1};
    } else {
      Y[e] = y0; Y[e + 1] = y1;
    }
    if (NORM) {
      a0 = __dadd_rn(a0, __dmul_rn(y0, y0));
      a1 = __dadd_rn(a1, __dmul_rn(y1, y1));
    }
  }
}

template <int W, bool NORM>
__global__ __launch_bounds__(256) void k_gs_update(double* Y, const double* const* __restrict__ V, int nb,
                                                   const double* __restrict__ C, int n, int rows_per, double* work) {
  constexpr int H = W / 2, R = 256 / H;
  __shared__ double cs[BLK_GS_NBMAX * W];
  __shared__ double red[R][W];
  const int t = threadIdx.x, c = t % H, rl = t / H;
  const int lo = blockIdx.x * rows_per, hi = min(n, lo + rows_per);
  for (int e = t; e < nb * W; e += 256) cs[e] = C[e];
  uintptr_t bits = reinterpret_cast<uintptr_t>(Y);
  for (int k = 0; k < nb; ++k) bits |= reinterpret_cast<uintptr_t>(V[k]);
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
  if ((bits & 15u) == 0) gs_update_rows<W, NORM, true>(Y, V, nb, cs, lo, hi, c, rl, a0, a1);
  else gs_update_rows<W, NORM, false>(Y, V, nb, cs, lo, hi, c, rl, a0, a1);
  if (NORM) {
    red[rl][2 * c] = a0;
    red[rl][2 * c + 1] = a1;
    __syncthreads();
    if (t < W) {
      double s = red[0][t];
      for (int r = 1; r < R; ++r) s = __dadd_rn(s, red[r][t]);
      work[(int64_t)blockIdx.x * W + t] = s;
    }
  }
}

bool block_gs_update(double* Y, const double* const* V, int nb, const double* C, int n, int w, double* norm2, double* work) {
  if (w != 16 && w != 32) throw std::runtime_error("block_gs_update: width is not 16 or 32");
  if (nb < 0 || n < 0 || !Y || (nb > 0 && (!V || !C)) || (norm2 && !work)) throw std::runtime_error("block_gs_update: bad argument");
  if (nb == 0) return norm2 ? block_coldot(Y, Y, n, w, norm2, work) : true;
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = block_coldot_nwg(n), rows_per = block_coldot_rows_per(n);
  for (int k0 = 0; k0 < nb; k0 += BLK_GS_NBMAX) {
    const int nk = std::min(BLK_GS_NBMAX, nb - k0);
    const bool norm = norm2 && k0 + nk == nb;         // the squares of the final values alone
    const double* const* Vk = V + k0;
    const double* Ck = C + (size_t)k0 * w;
#define BLK_UPD(W_, N_) hipLaunchKernelGGL((k_gs_update<W_, N_>), dim3(nwg), dim3(256), 0, s, Y, Vk, nk, Ck, n, rows_per, work)
    if (w == 16) { if (norm) BLK_UPD(16, true); else BLK_UPD(16, false); }
    else { if (norm) BLK_UPD(32, true); else BLK_UPD(32, false); }
#undef BLK_UPD
  }
  if (norm2) hipLaunchKernelGGL(k_coldot2, dim3(1), dim3(64), 0, s, work, nwg, w, norm2);
  HIPCHK(hipGetLastError());
  return true;
}

__global__ __launch_bounds__(256) void k_scale_cols(double* Out, const double* X, const double* __restrict__ c, int64_t tot,
                                                    int w, int vec) {
  const int64_t gs = (int64_t)gridDim.x * blockDim.x, g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vec) {
    for (int64_t e = g0; e < tot; e += gs) Out[e] = __dmul_rn(c[e & (w - 1)], X[e]);
    return;
  }
  for (int64_t p = g0; p < (tot >> 1); p += gs) {  // tot = n w is even; both entries lie in one row
    const int64_t e = 2 * p;
    const int j = (int)(e & (w - 1));
    const blk_d2 xv = *reinterpret_cast<const blk_d2*>(X + e);
    *reinterpret_cast<blk_d2*>(Out + e) = blk_d2{__dmul_rn(c[j], xv.x), __dmul_rn(c[j + 1], xv.y)};
  }
}

bool block_scale_cols(double* Out, const double* X, const double* c, int n, int w) {
  if (w != 16 && w != 32) throw std::runtime_error("block_scale_cols: width is not 16 or 32");
  if (n <= 0) return true;
  if (!Out || !X || !c) throw std::runtime_error("block_scale_cols: null argument");
  const int64_t tot = (int64_t)n * w;
  const int vec = blk_al16(Out) && blk_al16(X) ? 1 : 0;
  const int64_t work = vec ? tot / 2 : tot;
  const int grid = (int)std::min<int64_t>((work + 255) / 256, 8192);
  hipLaunchKernelGGL(k_scale_cols, dim3(grid), dim3(256), 0, (hipStream_t)get_stream(), Out, X, c, tot, w, vec);
  HIPCHK(hipGetLastError());
  return true;
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
