// Device primitives of the block (multi right-hand-side) entry points: PCMatApply_GenEO, MatMatMult_GenEO and
// KSPMatSolve_GenEO (block PCG and, -ksp_matsolve_type gmres, block GMRES) on the Chebyshev local solver
// (-geneo_block_width 16|32; block_dev.hip).
// Kept apart from backend.h, as cheb_dev.h is: optional on a backend.  core.cpp carries WORKING weak definitions of all of
// them, composed of backend.h primitives on scratch they allocate and free in the call (the host twin runs those; on the
// GPU GeneoSetKernelVariant("block_fused", 0) selects the composed forms); the HIP object's definitions override them.
//
// Slabs are row-major n x w blocks, w = 16 | 32 (leading dimension w).  Everything is stream-ordered: no synchronisation,
// no allocation, no atomics.  Every column is computed from its own entries alone, in a fixed row order: a column's result
// does not depend on its position in the slab or on its neighbours.
#pragma once

#include "backend.h"

namespace bk {

// The step of cheb_dir (cheb_dev.h) on slabs: Z, D, X, Out are c.n x w; (a, b) = (coef_k[2 s], coef_k[2 s + 1]) for all
// rows and columns of subdomain s; dscale (c.n, may be null) scales ROWS.  Same flags, same roundings
// (d = fl(fl(a z) + fl(b d)), x = fl(x + d), out = fl(dscale x)): column j equals cheb_dir on column j to the bit.
bool cheb_dir_block(const Chunks& c, const double* coef_k, int flags, const double* Z, double* D, double* X,
                    const double* dscale, double* Out, int w);

// Column-major (leading dimension ld >= n, m <= w columns) <-> slab.  Import zero-fills the slab's columns m .. w - 1;
// export writes n rows of the first m columns and nothing else.
bool block_import(const double* Xcm, int ld, int n, int m, double* Yrm, int w);
bool block_export(const double* Xrm, int w, int n, int m, double* Ycm, int ld);

// out[j] = sum_i X[i][j] Y[i][j], j < w, over n rows, in a fixed order for a given n: per-workgroup partials over
// consecutive row ranges, reduced in index order.  work: BLOCK_COLDOT_WG x w doubles of the caller.
constexpr int BLOCK_COLDOT_WG = 1024;
bool block_coldot(const double* X, const double* Y, int n, int w, double* out, double* work);

// Y[:, j] = fl(Y[:, j] + fl(c[j] X[:, j]))  and  P[:, j] = fl(Z[:, j] + fl(c[j] P[:, j])); c: w doubles on the device
bool block_axpy_cols(double* Y, const double* X, const double* c, int n, int w);
bool block_xpby_cols(double* P, const double* Z, const double* c, int n, int w);

// ---- Gram-Schmidt on slabs (the block GMRES of KSPMatSolve_GenEO).  V: nb slab pointers, an array on the DEVICE.
// The workgroups of block_coldot on n rows, and the rows each of them takes
inline int block_coldot_nwg(int n) {
  const int g = (n + 63) / 64;
  return g < 1 ? 1 : g > BLOCK_COLDOT_WG ? BLOCK_COLDOT_WG : g;
}
inline int block_coldot_rows_per(int n) {
  const int nwg = block_coldot_nwg(n);
  return ((n > 1 ? n : 1) + nwg - 1) / nwg;
}

// H[i w + j] = sum_r V_i[r][j] W[r][j], i < nb: row i has the bits of block_coldot(V_i, W) (its row ranges, lane map,
// rounded products and sums, and two-stage reduction), but the rows of W are read once per group of BLOCK_GS_GROUP slabs.
// work: block_coldot_nwg(n) x nb x w doubles of the caller (at most BLOCK_COLDOT_WG x nb x w).
constexpr int BLOCK_GS_GROUP = 8;
bool block_gs_dots(const double* const* V, int nb, const double* W, int n, int w, double* H, double* work);

// Y[:, j] = fl(Y[:, j] + fl(C[i w + j] V_i[:, j])) for i = 0 .. nb - 1 in that order, in one pass over Y: the bits of nb
// successive block_axpy_cols.  norm2 (w doubles, may be null): sum_r Y'[r][j]^2 of the result, the bits of
// block_coldot(Y', Y'); work (BLOCK_COLDOT_WG x w doubles) is needed with norm2 only.
bool block_gs_update(double* Y, const double* const* V, int nb, const double* C, int n, int w, double* norm2, double* work);

// Out[:, j] = fl(c[j] X[:, j]); Out may be X
bool block_scale_cols(double* Out, const double* X, const double* c, int n, int w);

// Y <- (L L^T)^-1 Y for n x w row-major Y, n <= 1024: the sweeps of bk::chol_solve on every column in ONE launch, per
// column the same operations in the same order (same bits).  false: n beyond the capacity, nothing done.
bool chol_solve_block(const double* L, const double* LT, int n, double* Y, int w);

}  // namespace bk
