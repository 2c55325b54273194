// HIP / CDNA4 (gfx950) kernel of the Chebyshev local solver (cheb_dev.h): the direction and solution update of one
// step for all subdomains of the rank, each with its own coefficients.
//
//   k_cheb_dir<FIRST, LAST>   one workgroup per chunk (at most 1024 rows of ONE subdomain).  The chunk's subdomain and
//                             its (a, b) arrive through scalar loads (the chunk index is the workgroup index) and are
//                             pinned wave-uniform; the rest is a stream: z, d, x in, d, x (and out) back -- 40 B per
//                             row, 48 B with out, 56 B with out and dscale; the first step reads z alone.  16-byte
//                             loads and stores on the even-aligned body of the chunk, scalar head and tail.
// d = fl(fl(a z) + fl(b d)) with contraction off: the bits of the composed form in core.cpp (block_colscale, axpy).
// Every element is read and written by one lane and no sum crosses lanes: results do not depend on the geometry.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "cheb_dev.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                 \
    }                                                                                      \
  } while (0)

// No contraction in this file: a z + b d is two rounded products and a rounded sum (HIP's __dmul_rn / __dadd_rn are the
// plain operators and would be fused under the compiler's default).
#pragma clang fp contract(off)

namespace bk {

typedef double cheb_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double cheb_uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

template <bool FIRST>
__device__ __forceinline__ void cheb_step(double a, double b, double zv, double& dv, double& xv) {
  if (FIRST) {
    dv = __dmul_rn(a, zv);
    xv = dv;
  } else {
    dv = __dadd_rn(__dmul_rn(a, zv), __dmul_rn(b, dv));
    xv = __dadd_rn(xv, dv);
  }
}

template <bool FIRST, bool LAST>
__device__ __forceinline__ void cheb_one(int64_t i, double a, double b, const double* z, double* d, double* x,
                                         const double* dscale, double* out) {
  double dv = 0.0, xv = 0.0;
  if (!FIRST) {
    dv = d[i];
    xv = x[i];
  }
  const double sv = (LAST && dscale) ? dscale[i] : 1.0;
  cheb_step<FIRST>(a, b, z[i], dv, xv);
  d[i] = dv;
  x[i] = xv;
  if (LAST) out[i] = dscale ? __dmul_rn(sv, xv) : xv;
}

// vec: every base pointer is 16-byte aligned, so element i of every array is 16-byte aligned exactly when i is even
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_cheb_dir(int nchunk, const int* __restrict__ start, const int* __restrict__ len,
                                                  const int* __restrict__ sub, const double* __restrict__ coef,
                                                  const double* z, double* d, double* x, const double* dscale,
                                                  double* out, int vec) {
  const int c = blockIdx.x;
  if (c >= nchunk) return;
  const int s = __builtin_amdgcn_readfirstlane(sub[c]);
  const int64_t r0 = start[c];
  const int n = len[c];
  const double a = cheb_uniform(coef[2 * (int64_t)s]);
  const double b = cheb_uniform(coef[2 * (int64_t)s + 1]);
  const int t = threadIdx.x;
  if (!vec) {
    for (int j = t; j < n; j += 256) cheb_one<FIRST, LAST>(r0 + j, a, b, z, d, x, dscale, out);
    return;
  }
  const int head = (int)(r0 & 1);                 // one scalar element in front of an odd start
  const int npair = (n - head) >> 1;              // (n >= 1, so n - head >= 0)
  const int64_t body = r0 + head;
  for (int p = t; p < npair; p += 256) {
    const int64_t i = body + 2 * (int64_t)p;      // even, and i + 1 <= r0 + n - 1
    const cheb_d2 zv = *reinterpret_cast<const cheb_d2*>(z + i);
    cheb_d2 dv = {0.0, 0.0}, xv = {0.0, 0.0}, sv = {1.0, 1.0};
    if (!FIRST) {
      dv = *reinterpret_cast<const cheb_d2*>(d + i);
      xv = *reinterpret_cast<const cheb_d2*>(x + i);
    }
    if (LAST && dscale) sv = *reinterpret_cast<const cheb_d2*>(dscale + i);
    double d0 = dv.x, d1 = dv.y, x0 = xv.x, x1 = xv.y;
    cheb_step<FIRST>(a, b, zv.x, d0, x0);
    cheb_step<FIRST>(a, b, zv.y, d1, x1);
    *reinterpret_cast<cheb_d2*>(d + i) = cheb_d2{d0, d1};
    *reinterpret_cast<cheb_d2*>(x + i) = cheb_d2{x0, x1};
    if (LAST) {
      if (dscale) *reinterpret_cast<cheb_d2*>(out + i) = cheb_d2{__dmul_rn(sv.x, x0), __dmul_rn(sv.y, x1)};
      else *reinterpret_cast<cheb_d2*>(out + i) = cheb_d2{x0, x1};
    }
  }
  if (t == 0 && head) cheb_one<FIRST, LAST>(r0, a, b, z, d, x, dscale, out);
  if (t == 64 && ((n - head) & 1)) cheb_one<FIRST, LAST>(r0 + n - 1, a, b, z, d, x, dscale, out);
}

bool cheb_dir(const Chunks& c, const double* coef_k, int flags, const double* z, double* d, double* x,
              const double* dscale, double* out) {
  if (c.nchunk <= 0) return true;
  const bool first = (flags & 1) != 0, last = (flags & 2) != 0;
  if (!coef_k || !z || !d || !x || (last && !out)) throw std::runtime_error("cheb_dir: null argument");
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const int vec = al(z) && al(d) && al(x) && (!last || (al(out) && (!dscale || al(dscale)))) ? 1 : 0;
  hipStream_t s = (hipStream_t)get_stream();
  const dim3 grid(c.nchunk), block(256);
#define CHEB_LAUNCH(F, L) \
  hipLaunchKernelGGL((k_cheb_dir<F, L>), grid, block, 0, s, c.nchunk, c.start, c.len, c.sub, coef_k, z, d, x, dscale, out, vec)
  if (first && last) CHEB_LAUNCH(true, true);
  else if (first) CHEB_LAUNCH(true, false);
  else if (last) CHEB_LAUNCH(false, true);
  else CHEB_LAUNCH(false, false);
#undef CHEB_LAUNCH
  HIPCHK(hipGetLastError());
  return true;
}

}  // namespace bk
