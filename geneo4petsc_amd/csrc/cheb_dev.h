// Device primitives of the Chebyshev local solver (-dls1_ksp_type chebyshev; cheb_dev.hip and backend_hip.hip).
// Kept apart from backend.h: both are optional on a backend.  core.cpp carries weak definitions that the HIP objects
// override: cheb_dir's is WORKING (the same arithmetic composed of backend.h primitives, on scratch it allocates and frees
// in the call), cheb_residual's answers "not available" and the caller runs bk::spmv and bk::axpy instead.
#pragma once

#include "backend.h"

namespace bk {

// One step of the direction / solution update, per subdomain s of c with (a, b) = (coef_k[2 s], coef_k[2 s + 1]):
//   flags bit 0 clear:  d = a z + b d ;  x += d
//   flags bit 0 set:    d = a z ;        x  = d        (first step: neither d nor x is read)
//   flags bit 1 set:    additionally out = x, or out = dscale .* x when dscale is non-null (last step)
// a z + b d is evaluated as fl(fl(a z) + fl(b d)), no contraction, by both definitions: they agree to the bit.
// Stream-ordered, no synchronisation, no atomics; every element is touched by exactly one lane.  out may alias any
// buffer but z, d and x (it is written last, element by element).  The composed definition needs c.suboff[0] == 0.
bool cheb_dir(const Chunks& c, const double* coef_k /* nsub x 2, device */, int flags, const double* z, double* d,
              double* x, const double* dscale, double* out);

// r_out = r_in - A d through the sliced traversal of bk::spmv (same column source: 16-bit offsets or offset-coded
// slices where the matrix carries them; same summation order and one rounded subtraction, so the bits of bk::spmv followed
// by bk::axpy(r, -1, q): tests/test_gpu_cheb_local_solver.py compares whole applies of the two forms bit for bit).
// r_out must not be r_in or d.  false: nothing done (matrix off the wave-per-slice path, or a backend without it).
bool cheb_residual(const Csr& a, const double* d, const double* r_in, double* r_out);

}  // namespace bk
