// Device factorisation and blocked triangular sweeps of the replicated coarse operator E, for any dimE (coarse_dev.hip).
// Kept apart from backend.h: these two are optional on a backend.  core.cpp carries weak definitions that answer "not
// available" (false, nothing touched); the HIP object overrides them.  A caller that gets false takes the host path.
#pragma once

namespace bk {

// E = L L^T, n x n row-major on the device, block size nb (a multiple of 16 in 16 .. 256).  L: lower factor, strict upper
// part exactly zero; LT: its bitwise transpose -- the pair bk::chol_solve reads.  E may be L (in place).  *status (device):
// 0, or 1 + the index of the first pivot with !(d > 0), after which L and LT hold no factor.  Stream-ordered, no
// synchronisation, fixed summation orders (the same input gives the same bits).
bool coarse_factor(const double* E, int n, int nb, double* L, double* LT, int* status);

// y <- (L L^T)^-1 y in place, any n: per block row one matrix-vector launch over many workgroups and one
// one-workgroup substitution on nb unknowns.  Stream-ordered, no synchronisation, fixed summation orders.
bool coarse_solve(const double* L, const double* LT, int n, int nb, double* y);

// Y <- (L L^T)^-1 Y in place on the n x w row-major slab Y (w = 16 | 32, leading dimension w), any n: the two launches per
// block row of coarse_solve, each for all w columns together (4 ceil(n / nb) - 2 launches per slab).  Every element is one
// accumulation chain over its own column in a fixed order: a column's bits depend neither on its position, nor on its
// neighbours, nor on w, and a zero column stays +0.  Stream-ordered, no synchronisation, no allocation, no atomics.
bool coarse_solve_block(const double* L, const double* LT, int n, int nb, double* Y, int w);

}  // namespace bk
