// Device primitives of the right-preconditioned and flexible GMRES of KSPSolve_GenEO (-ksp_pc_side right, -ksp_type
// fgmres; krylov_dev.hip): the two Gram-Schmidt passes of a step on single vectors.
// Kept apart from backend.h, as block_dev.h is: optional on a backend.  core.cpp carries WORKING weak definitions of both,
// composed of backend.h primitives -- one bk::dot per basis vector; one bk::axpy per basis vector and bk::dot for the norm
// -- which the host twin runs and GeneoSetKernelVariant("krylov_fused", 0) selects on the GPU; the HIP object's
// definitions override them.  The two forms agree within rounding, not to the bit: bk::dot has its own reduction tree and
// bk::axpy may contract its multiply-add.
//
// Vectors are contiguous FP64.  V is a table of nb vector pointers ON THE DEVICE.  Everything is stream-ordered: no
// synchronisation, no allocation, no atomics.  Loads are 16 bytes wide where every vector of a pass is 16-byte aligned,
// scalar otherwise and at a ragged end; the lanes read the same entries and sum them in the same order either way.
//
// Bytes moved by a step over nb basis vectors of n rows, from the definitions: fused (2 nb + ceil(nb / 8) + 2) 8 n with 2
// host round trips; composed (5 nb + 2) 8 n with nb + 2 round trips.
#pragma once

#include "backend.h"

namespace bk {

// A pass splits the n rows into consecutive ranges of vec_dot_rows_per(n) rows (even, so that every range starts on a
// 16-byte boundary of an aligned vector), one workgroup each: VEC_DOT_RANGE rows -- one sweep of a workgroup, 256 lanes
// with two entries each -- up to VEC_DOT_WG ranges, longer ranges beyond.
constexpr int VEC_DOT_WG = 1024, VEC_DOT_RANGE = 512;
inline int vec_dot_rows_per(int n) {
  const int g0 = (n + VEC_DOT_RANGE - 1) / VEC_DOT_RANGE;
  const int g = g0 < 1 ? 1 : g0 > VEC_DOT_WG ? VEC_DOT_WG : g0;
  const int r = (int)((((long long)(n > 1 ? n : 1) + g - 1) / g + 1) & ~1ll);
  return r;
}
inline int vec_dot_nwg(int n) {
  const int r = vec_dot_rows_per(n);
  const int g = (int)(((long long)n + r - 1) / r);
  return g < 1 ? 1 : g;
}

// H[i] = sum_r V_i[r] W[r], i < nb.  Per-workgroup partials over the row ranges above (rounded products and sums, a fixed
// lane map and reduction tree), summed in index order by a second small launch.  W is read once per group of VEC_GS_GROUP
// vectors, whose accumulators stay in registers.  H[i] depends on V_i, W and n alone: not on nb, not on i's position in
// its group, not on the 8-byte alignment of any pointer.
// work: vec_dot_nwg(n) x nb doubles of the caller.
constexpr int VEC_GS_GROUP = 8;
bool vec_gs_dots(const double* const* V, int nb, const double* W, int n, double* H, double* work);

// Y[r] = fl(Y[r] + fl(C[i] V_i[r])) for i = 0 .. nb - 1 in that order, in one pass over Y (C: nb doubles on the device).
// norm2 (one double, may be null): sum_r Y'[r]^2 of the result, with the bits vec_gs_dots(&Y', 1, Y') gives; work
// (vec_dot_nwg(n) doubles) is needed, and written, with norm2 only.
bool vec_gs_update(double* Y, const double* const* V, int nb, const double* C, int n, double* norm2, double* work);

// The step of the flexible CG (-ksp_type fcg) with its coefficient on the device.  S: two doubles ON THE DEVICE, [eta, pi]
// = [(A p, p), (r, p)].  alpha = pi / eta (correctly rounded); x[r] = fl(x[r] + fl(alpha p[r])), r[r] = fl(r[r] -
// fl(alpha w[r])) in one pass, with the row ranges, lane map and load paths of vec_gs_update.  If eta is not positive (zero,
// negative, NaN) nothing is written to x or r.  norm2 (one double, may be null): sum_r r'[r]^2 of r as the call leaves it,
// with the bits vec_gs_dots(&r', 1, r') gives; work (vec_dot_nwg(n) doubles) is needed, and written, with norm2 only.
// Bytes, from the definitions: fused 6 x 8 n, one launch (two with norm2), no download; composed (core.cpp: download S,
// bk::axpy, bk::axpy, bk::dot) 8 x 8 n, three launches and a download.
bool vec_fcg_step(double* x, double* r, const double* p, const double* w, const double* S, int n, double* norm2, double* work);

// true where the functions above are the kernels (the HIP object), false where they are core.cpp's composed forms: the
// driver then runs those on its host copies of the pointer table and the coefficients, and counts its passes as composed
bool vec_gs_kernels();

}  // namespace bk
