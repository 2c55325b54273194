// HIP / CDNA4 (gfx950) kernels of the right-preconditioned and flexible GMRES (krylov_dev.h): the Gram-Schmidt passes of a
// step on single contiguous FP64 vectors.
//
//   k_vec_dots1 / k_vec_dots2  h_i = (v_i, w) for up to VEC_GS_GROUP vectors per pass over w.  Workgroup blockIdx.x takes
//                              the rows [x r, (x + 1) r), r = vec_dot_rows_per(n) (even); lane t the pairs of entries
//                              2 t, 2 t + 1 (+ 512 j) of that range: one 16-byte load per vector where every pointer of
//                              the group is 16-byte aligned, two 8-byte loads otherwise and one at a ragged end -- the
//                              same entries, products and sums either way.  Every vector of the group (blockIdx.y) has its
//                              own two accumulators (even and odd entries), added, reduced over the wave by shuffles and
//                              over the four waves through LDS in index order.  k_vec_dots2 adds the partials of a vector
//                              in index order, one thread per vector.  No atomics: the bits depend on v_i, w and n alone.
//   k_vec_update               y <- fl(y + fl(c_i v_i)), i = 0 .. nb - 1 in that order, on the entries a lane of
//                              k_vec_dots1 owns, so that the squares of the result are summed in its order (NORM): the
//                              partials of vec_gs_dots(&y', 1, y').  The coefficients of a launch (at most VEC_GS_NBMAX
//                              vectors; the wrapper splits longer lists) sit in LDS.
//   k_vec_fcg_step             the step of the flexible CG on the rows and lanes of k_vec_update: every workgroup reads
//                              [eta, pi] and forms alpha = pi / eta; x <- fl(x + fl(alpha p)), r <- fl(r - fl(alpha w)),
//                              and (NORM) the partials of vec_gs_dots(&r', 1, r').  eta not positive: no store.
//   k_vec_sum_staged           k_vec_dots2's sum of one vector's partials, in its order and to its bits, from LDS.
// Products and sums are rounded one by one (contraction off): the numpy expressions of the tests to the bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "krylov_dev.h"

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

typedef double kry_d2 __attribute__((ext_vector_type(2)));

constexpr int KRY_THREADS = 256, KRY_WAVES = KRY_THREADS / 64;
static_assert(VEC_DOT_RANGE == 2 * KRY_THREADS, "a range of the smallest length is one sweep of a workgroup");

// entries e, e + 1 of p (the second one only where `pair`): VEC needs p + e 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void kry_load2(const double* p, int64_t e, bool pair, double& x0, double& x1) {
  if (VEC && pair) {
    const kry_d2 v = *reinterpret_cast<const kry_d2*>(p + e);
    x0 = v.x;
    x1 = v.y;
  } else {
    x0 = p[e];
    x1 = pair ? p[e + 1] : 0.0;
  }
}

// sum over the 64 lanes of a wave, a fixed tree; the result is in lane 0
__device__ __forceinline__ double kry_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off, 64));
  return v;
}

template <bool VEC>
__device__ __forceinline__ void vec_dots_rows(const double* const (&vp)[VEC_GS_GROUP], int ng, const double* Wv, int64_t lo,
                                              int64_t hi, int t, double (&a0)[VEC_GS_GROUP], double (&a1)[VEC_GS_GROUP]) {
  for (int64_t e = lo + 2 * t; e < hi; e += 2 * KRY_THREADS) {
    const bool pair = e + 1 < hi;
    double w0, w1;
    kry_load2<VEC>(Wv, e, pair, w0, w1);
#pragma unroll
    for (int g = 0; g < VEC_GS_GROUP; ++g) {
      if (g < ng) {                                    // (uniform)
        double x0, x1;
        kry_load2<VEC>(vp[g], e, pair, x0, x1);
        a0[g] = __dadd_rn(a0[g], __dmul_rn(x0, w0));
        if (pair) a1[g] = __dadd_rn(a1[g], __dmul_rn(x1, w1));
      }
    }
  }
}

__global__ __launch_bounds__(KRY_THREADS) void k_vec_dots1(const double* const* __restrict__ V, int nb,
                                                           const double* __restrict__ Wv, int n, int rows_per, int nwg,
                                                           double* __restrict__ work) {
  constexpr int G = VEC_GS_GROUP;
  __shared__ double part[G][KRY_WAVES];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * rows_per, hi = min((int64_t)n, lo + rows_per);
  const int i0 = blockIdx.y * G, ng = min(G, nb - i0);
  const double* vp[G];
  uintptr_t bits = reinterpret_cast<uintptr_t>(Wv);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    vp[g] = V[i0 + min(g, ng - 1)];
    bits |= reinterpret_cast<uintptr_t>(vp[g]);
  }
  double a0[G], a1[G];
#pragma unroll
  for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0;
  if ((bits & 15u) == 0) vec_dots_rows<true>(vp, ng, Wv, lo, hi, t, a0, a1);
  else vec_dots_rows<false>(vp, ng, Wv, lo, hi, t, a0, a1);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double s = kry_wave_sum(__dadd_rn(a0[g], a1[g]));
    if ((t & 63) == 0) part[g][t >> 6] = s;
  }
  __syncthreads();
  if (t < ng) {
    double s = part[t][0];
#pragma unroll
    for (int v = 1; v < KRY_WAVES; ++v) s = __dadd_rn(s, part[t][v]);
    work[(int64_t)(i0 + t) * nwg + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void k_vec_dots2(const double* __restrict__ work, int nwg, int nb, double* __restrict__ H) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nb) return;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s = __dadd_rn(s, work[(int64_t)i * nwg + g]);
  H[i] = s;
}

bool vec_gs_dots(const double* const* V, int nb, const double* Wv, int n, double* H, double* work) {
  if (nb < 0 || n < 0 || (nb > 0 && (!V || !Wv || !H || !work))) throw std::runtime_error("vec_gs_dots: bad argument");
  if (nb == 0) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = vec_dot_nwg(n), rows_per = vec_dot_rows_per(n);
  const dim3 grid(nwg, (nb + VEC_GS_GROUP - 1) / VEC_GS_GROUP);
  hipLaunchKernelGGL(k_vec_dots1, grid, dim3(KRY_THREADS), 0, s, V, nb, Wv, n, rows_per, nwg, work);
  hipLaunchKernelGGL(k_vec_dots2, dim3((nb + 63) / 64), dim3(64), 0, s, work, nwg, nb, H);
  HIPCHK(hipGetLastError());
  return true;
}

bool vec_gs_kernels() { return true; }

constexpr int VEC_GS_NBMAX = 64;

template <bool NORM, bool VEC>
__device__ __forceinline__ void vec_update_rows(double* Y, const double* const* __restrict__ V, int nb, const double* cs,
                                                int64_t lo, int64_t hi, int t, double& a0, double& a1) {
  for (int64_t e = lo + 2 * t; e < hi; e += 2 * KRY_THREADS) {
    const bool pair = e + 1 < hi;
    double y0, y1;
    kry_load2<VEC>(Y, e, pair, y0, y1);
#pragma unroll 4
    for (int k = 0; k < nb; ++k) {
      double x0, x1;
      kry_load2<VEC>(V[k], e, pair, x0, x1);
      y0 = __dadd_rn(y0, __dmul_rn(cs[k], x0));
      if (pair) y1 = __dadd_rn(y1, __dmul_rn(cs[k], x1));
    }
    if (VEC && pair) {
      *reinterpret_cast<kry_d2*>(Y + e) = kry_d2{y0, y1};
    } else {
      Y[e] = y0;
      if (pair) Y[e + 1] = y1;
    }
    if (NORM) {
      a0 = __dadd_rn(a0, __dmul_rn(y0, y0));
      if (pair) a1 = __dadd_rn(a1, __dmul_rn(y1, y1));
    }
  }
}

template <bool NORM>
__global__ __launch_bounds__(KRY_THREADS) void k_vec_update(double* Y, const double* const* __restrict__ V, int nb,
                                                            const double* __restrict__ C, int n, int rows_per, double* work) {
  __shared__ double cs[VEC_GS_NBMAX];
  __shared__ double part[KRY_WAVES];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * rows_per, hi = min((int64_t)n, lo + rows_per);
  if (t < nb) cs[t] = C[t];
  uintptr_t bits = reinterpret_cast<uintptr_t>(Y);
  for (int k = 0; k < nb; ++k) bits |= reinterpret_cast<uintptr_t>(V[k]);
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
  if ((bits & 15u) == 0) vec_update_rows<NORM, true>(Y, V, nb, cs, lo, hi, t, a0, a1);
  else vec_update_rows<NORM, false>(Y, V, nb, cs, lo, hi, t, a0, a1);
  if (NORM) {
    const double s = kry_wave_sum(__dadd_rn(a0, a1));
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
      double r = part[0];
#pragma unroll
      for (int v = 1; v < KRY_WAVES; ++v) r = __dadd_rn(r, part[v]);
      work[blockIdx.x] = r;
    }
  }
}

bool vec_gs_update(double* Y, const double* const* V, int nb, const double* C, int n, double* norm2, double* work) {
  if (nb < 0 || n < 0 || !Y || (nb > 0 && (!V || !C)) || (norm2 && !work)) throw std::runtime_error("vec_gs_update: bad argument");
  if (nb == 0 && !norm2) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = vec_dot_nwg(n), rows_per = vec_dot_rows_per(n);
  int k0 = 0;
  do {                                                // nb == 0 with norm2: one launch that sums the squares of Y as it is
    const int nk = std::min(VEC_GS_NBMAX, nb - k0);
    const bool norm = norm2 && k0 + nk == nb;         // the squares of the final values alone
    const double* const* Vk = V + k0;
    const double* Ck = C + k0;
    if (norm) hipLaunchKernelGGL((k_vec_update<true>), dim3(nwg), dim3(KRY_THREADS), 0, s, Y, Vk, nk, Ck, n, rows_per, work);
    else hipLaunchKernelGGL((k_vec_update<false>), dim3(nwg), dim3(KRY_THREADS), 0, s, Y, Vk, nk, Ck, n, rows_per, work);
    k0 += nk;
  } while (k0 < nb);
  if (norm2) hipLaunchKernelGGL(k_vec_dots2, dim3(1), dim3(64), 0, s, work, nwg, 1, norm2);
  HIPCHK(hipGetLastError());
  return true;
}

// The step of the flexible CG: alpha = pi / eta from the two doubles S on the device, x += alpha p, r -= alpha w on the
// entries a lane of k_vec_update owns.  GO false (eta not positive, or NaN): nothing is stored, and the squares summed are
// those of r as it is.
template <bool NORM, bool VEC>
__device__ __forceinline__ void vec_step_rows(double* X, double* R, const double* __restrict__ P, const double* __restrict__ Wv,
                                              bool go, double alpha, int64_t lo, int64_t hi, int t, double& a0, double& a1) {
  for (int64_t e = lo + 2 * t; e < hi; e += 2 * KRY_THREADS) {
    const bool pair = e + 1 < hi;
    double r0, r1;
    kry_load2<VEC>(R, e, pair, r0, r1);
    if (go) {
      double x0, x1, p0, p1, w0, w1;
      kry_load2<VEC>(X, e, pair, x0, x1);
      kry_load2<VEC>(P, e, pair, p0, p1);
      kry_load2<VEC>(Wv, e, pair, w0, w1);
      x0 = __dadd_rn(x0, __dmul_rn(alpha, p0));
      r0 = __dsub_rn(r0, __dmul_rn(alpha, w0));
      if (pair) {
        x1 = __dadd_rn(x1, __dmul_rn(alpha, p1));
        r1 = __dsub_rn(r1, __dmul_rn(alpha, w1));
      }
      if (VEC && pair) {
        *reinterpret_cast<kry_d2*>(X + e) = kry_d2{x0, x1};
        *reinterpret_cast<kry_d2*>(R + e) = kry_d2{r0, r1};
      } else {
        X[e] = x0;
        R[e] = r0;
        if (pair) {
          X[e + 1] = x1;
          R[e + 1] = r1;
        }
      }
    }
    if (NORM) {
      a0 = __dadd_rn(a0, __dmul_rn(r0, r0));
      if (pair) a1 = __dadd_rn(a1, __dmul_rn(r1, r1));
    }
  }
}

template <bool NORM>
__global__ __launch_bounds__(KRY_THREADS) void k_vec_fcg_step(double* X, double* R, const double* __restrict__ P,
                                                              const double* __restrict__ Wv, const double* __restrict__ S,
                                                              int n, int rows_per, double* work) {
  __shared__ double part[KRY_WAVES];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * rows_per, hi = min((int64_t)n, lo + rows_per);
  const double eta = S[0], pi = S[1];
  const bool go = eta > 0.0;                           // (uniform) false for a NaN too
  if (!NORM && !go) return;
  const double alpha = go ? __ddiv_rn(pi, eta) : 0.0;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(P) |
                         reinterpret_cast<uintptr_t>(Wv);
  double a0 = 0.0, a1 = 0.0;
  if ((bits & 15u) == 0) vec_step_rows<NORM, true>(X, R, P, Wv, go, alpha, lo, hi, t, a0, a1);
  else vec_step_rows<NORM, false>(X, R, P, Wv, go, alpha, lo, hi, t, a0, a1);
  if (NORM) {
    const double s = kry_wave_sum(__dadd_rn(a0, a1));
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
      double r = part[0];
#pragma unroll
      for (int v = 1; v < KRY_WAVES; ++v) r = __dadd_rn(r, part[v]);
      work[blockIdx.x] = r;
    }
  }
}

// The sum k_vec_dots2 makes of the partials of ONE vector -- 0 + work[0] + work[1] + ... in index order, the same bits --
// with the partials staged in LDS by the whole workgroup first: the one thread that adds them then waits for LDS, not for
// a global load per term.  nwg <= VEC_DOT_WG.
__global__ __launch_bounds__(KRY_THREADS) void k_vec_sum_staged(const double* __restrict__ work, int nwg, double* __restrict__ out) {
  __shared__ double part[VEC_DOT_WG];
  for (int g = threadIdx.x; g < nwg; g += KRY_THREADS) part[g] = work[g];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll 16
    for (int g = 0; g < nwg; ++g) s = __dadd_rn(s, part[g]);
    out[0] = s;
  }
}

bool vec_fcg_step(double* x, double* r, const double* p, const double* w, const double* S, int n, double* norm2, double* work) {
  if (n < 0 || !x || !r || !p || !w || !S || (norm2 && !work)) throw std::runtime_error("vec_fcg_step: bad argument");
  if (n == 0 && !norm2) return true;
  hipStream_t s = (hipStream_t)get_stream();
  const int nwg = vec_dot_nwg(n), rows_per = vec_dot_rows_per(n);
  if (nwg > VEC_DOT_WG) throw std::runtime_error("vec_fcg_step: more partial sums than k_vec_sum_staged holds");
  if (norm2) {
    hipLaunchKernelGGL((k_vec_fcg_step<true>), dim3(nwg), dim3(KRY_THREADS), 0, s, x, r, p, w, S, n, rows_per, work);
    hipLaunchKernelGGL(k_vec_sum_staged, dim3(1), dim3(KRY_THREADS), 0, s, work, nwg, norm2);
  } else {
    hipLaunchKernelGGL((k_vec_fcg_step<false>), dim3(nwg), dim3(KRY_THREADS), 0, s, x, r, p, w, S, n, rows_per, work);
  }
  HIPCHK(hipGetLastError());
  return true;
}

}  // namespace bk
