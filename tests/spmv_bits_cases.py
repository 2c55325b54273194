"""Cases of tests/test_gpu_spmv_bits.py and tests/golden/make_spmv_bits_goldens.py: the single-vector sparse products and
their fused epilogues, output by output, as sha256 digests of the result bytes.

Every summation order of these kernels is fixed, so a launch gives the same bits on every run of one build; the goldens
record them for one compiler (the string the compiler leaves in libgeneopc.so), and a refactor of the kernels has to
reproduce them.  The shapes are the smallest that reach each branch of the sliced kernels:

  band k x n     every row exactly k entries.  k <= 8: the two-latency narrow forms; 9 .. 15: the predicated form of the
                 companion, the 4-step loop plus tail of the FP64 kernels; from k = 16 on the average slice width reaches the
                 workgroup-per-slice threshold, so 16, 18 and 23 run k_spmv_sell_wide and the WPS = 4 companion (k = 23
                 under kind 101: at 20 per row a small matrix would otherwise leave the slices for the lanes-per-row
                 kernel).  n = 130 and 257: a partial last slice, a last workgroup of fewer than four slices.  n = 1.
  mixed k        64 rows of k = 16, 18, 23 entries in front of 193 rows of 3: the average stays under 16, so the first slice
                 runs the WAVE-per-slice kernels at that width -- the predicated form at 16, four full rounds of the 4-step
                 loop plus a 2- and a 3-entry tail at 18 and 23.
  ragged         5000 rows, 8 entries per row on average (7 random ones and the diagonal): slice width and row length differ
                 (padding); the slices are 11 .. 18 wide, 14.7 on average -- under the workgroup-per-slice threshold, so the
                 wave-per-slice kernels run their predicated form and their 4-step loop on them.
  wide 30 / 45   n = 640, band of half-width 300, kind 101: workgroup-per-slice kernels, FP64 and companion, with the column
                 span of a 16-bit base at its default, 450 (two bases) and 40 (32-bit fallback).
  stencil        12 x 12 x 12 7-point block in natural order: offset-coded slices (all-present and bit-walk rows), with the
                 coded path on and off.
  kinds 21 / 31  the cached and the non-temporal stream of k_spmv_sell on the 257-row case.
  large          700 000 rows x 6: the smallest at which the padded entry count crosses both non-temporal thresholds
                 (12 B x entries > 48 MB, 6 B x entries >= 24 MB) and the FP64 product reads the 16-bit columns.
  block 16 / 20  the epilogues of k_spmm_sell, k_spmm_sell_wide (16 columns) and k_spmm (20 columns)."""
import hashlib
import os
import re

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmv_bits.json")
W = 0.61


def compiler_string(lib_path):
    """what the compiler wrote into the library (host and device .comment sections)"""
    with open(lib_path, "rb") as f:
        found = set(re.findall(rb"[ -~]*clang version [ -~]+", f.read()))
    return " | ".join(sorted(s.decode().strip() for s in found))


def band_fixed(n, k, half_width, seed):
    """exactly k entries per row, increasing columns within `half_width` of the diagonal"""
    rng = np.random.default_rng(seed)
    window = min(n, 2 * half_width + 1)
    assert k <= window
    r = np.arange(n)
    start = np.clip(r - half_width, 0, n - window)
    cols = start[:, None] + np.cumsum(rng.integers(1, window // k + 1, size=(n, k)), axis=1) - 1
    vals = (rng.random((n, k)) + 0.25) * rng.choice([-1.0, 1.0], size=(n, k))
    a = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(n + 1) * k), shape=(n, n))
    a.sort_indices()
    assert np.all(np.diff(a.indptr) == k) and a.indices.max() < n
    return a


def mixed(k, seed):
    """64 rows of k entries, then 193 rows of 3"""
    top = band_fixed(257, k, 60, seed)[:64]
    rest = band_fixed(257, 3, 60, seed + 1)[64:]
    a = sp.vstack([top, rest], format="csr")
    a.sort_indices()
    return a


def band_random(n, per_row, half_width, seed):
    rng = np.random.default_rng(seed)
    nnz = n * per_row
    rows = rng.integers(0, n, size=nnz)
    cols = np.clip(rows + rng.integers(-half_width, half_width + 1, size=nnz), 0, n - 1)
    a = (sp.csr_matrix((rng.random(nnz) - 0.5, (rows, cols)), shape=(n, n)) + sp.diags(rng.random(n) + 1.0)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def ragged(n, per_row, seed):
    rng = np.random.default_rng(seed)
    nnz = n * per_row
    a = (sp.csr_matrix((rng.random(nnz) - 0.5, (rng.integers(0, n, size=nnz), rng.integers(0, n, size=nnz))), shape=(n, n))
         + sp.diags(rng.random(n) + 1.0)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def stencil7(nx, ny, nz, seed):
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    i = np.arange(n)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols = [i], [i]
    for off, keep in ((-1, x > 0), (1, x < nx - 1), (-nx, y > 0), (nx, y < ny - 1), (-nx * ny, z > 0), (nx * ny, z < nz - 1)):
        rows.append(i[keep])
        cols.append(i[keep] + off)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (rng.random(len(rows)) + 0.5) * rng.choice([-1.0, 1.0], size=len(rows))
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a.sort_indices()
    return a


# name -> (matrix builder, kind, GENEO_LP_SPAN_MAX or None, offset-coded path on, block columns (0: vectors only))
CASES = {}
for _n in (130, 257):
    for _k in (1, 3, 4, 7, 8, 9, 12, 16, 18, 23):
        CASES["band_k%d_n%d" % (_k, _n)] = (lambda n=_n, k=_k: band_fixed(n, k, 40, 100 * k + n), 101 if _k >= 20 else 1, None, 1, 0)
CASES["band_k1_n1"] = (lambda: band_fixed(1, 1, 40, 5), 1, None, 1, 0)
for _k in (16, 18, 23):
    CASES["mixed_k%d" % _k] = (lambda k=_k: mixed(k, 300 + k), 1, None, 1, 0)
CASES["ragged_5000_avg8"] = (lambda: ragged(5000, 7, 7), 1, None, 1, 0)
for _per in (30, 45):
    for _span in (None, 450, 40):
        CASES["wide_%d_span_%s" % (_per, _span or "default")] = (lambda p=_per: band_random(640, p, 300, 31 + p), 101, _span, 1, 0)
CASES["stencil_12_coded"] = (lambda: stencil7(12, 12, 12, 9), 1, None, 1, 0)
CASES["stencil_12_stored"] = (lambda: stencil7(12, 12, 12, 9), 1, None, 0, 0)
CASES["band_k7_n257_kind21"] = (lambda: band_fixed(257, 7, 40, 957), 21, None, 1, 0)
CASES["band_k7_n257_kind31"] = (lambda: band_fixed(257, 7, 40, 957), 31, None, 1, 0)
CASES["large_700000_k6"] = (lambda: band_fixed(700000, 6, 15000, 51), 1, None, 1, 0)
CASES["block16_band_k7_n257"] = (lambda: band_fixed(257, 7, 40, 957), 1, None, 1, 16)
CASES["block16_wide_45"] = (lambda: band_random(640, 45, 300, 76), 101, None, 1, 16)
CASES["block20_ragged_5000_avg8"] = (lambda: ragged(5000, 7, 7), 1, None, 1, 20)


def _raw(lib, call, h, epi, n, X, B, Z, dinv, m=None):
    """one fused launch through the C ABI (Spmv.fused / fused_single always pass a z to EPI_PRE; this takes None too);
    returns (y, z or None)"""
    from geneo4petsc_amd.pc import DeviceVector
    dev = lambda v: DeviceVector.from_host(lib, np.ascontiguousarray(v, dtype=np.float64).ravel()) if v is not None else None
    xd, bd, zd, dd = dev(X), dev(B), dev(Z), dev(dinv)
    yd = DeviceVector(lib, n * (m or 1))
    p = lambda v: v.ptr if v is not None else None
    args = (h.h, int(epi), p(xd), yd.ptr) + ((int(m),) if m else ()) + (p(bd), p(zd), p(dd), float(W))
    assert call(*args) == 0, lib.PCGenEOGetError(None).decode()
    return yd.to_host(), (zd.to_host() if zd is not None else None)


def run_case(lib, name):
    """-> (matrix, inputs, {output name: array}) of one case, in launch order"""
    from geneo4petsc_amd.pc import Spmv
    build, kind, span, coded, m = CASES[name]
    a = build()
    n = a.shape[0]
    rng = np.random.default_rng(len(name) + n)
    shape = (n, m) if m else (n,)
    X, B, Z = rng.random(shape) - 0.5, rng.random(shape) - 0.5, rng.random(shape) - 0.5
    dinv = rng.random(n) + 0.5
    out = {}
    old_span = os.environ.get("GENEO_LP_SPAN_MAX")
    if span is not None:
        os.environ["GENEO_LP_SPAN_MAX"] = str(span)       # read by the library when the companion is built
    lib.GeneoSetSpmvKind(kind)
    assert lib.GeneoSetKernelVariant(b"sell_offsets", coded) == 0
    try:
        h = Spmv(a, lib)
        if m:
            for epi, kw in ((1, dict(X=X, B=B)), (2, dict(X=X, Z=Z)), (3, dict(X=X, B=B, dinv=dinv)),
                            (5, dict(X=X, B=B, Z=Z, dinv=dinv))):
                out["fused%d" % epi] = h.fused(epi, w=W, **kw)[0]
            out["fused4_y"], out["fused4_z"] = h.fused(4, B=B, dinv=dinv, w=W)
            out["fused4_no_z"] = _raw(lib, lib.GeneoSpmmFused, h, 4, n, None, B, None, dinv, m)[0]
        else:
            out["apply"] = h.apply(X)
            if kind in (21, 31):              # the stream variants concern the plain FP64 product only
                h.destroy()
                return a, (X, B, Z, dinv), out
            for pre, call in (("fused", lib.GeneoSpmmFused), ("single", lib.GeneoSpmvFusedSingle)):
                mm = 1 if pre == "fused" else None
                if pre == "single":
                    out["single0"] = h.fused_single(0, X=X)[0]        # builds the companion
                out[pre + "1"] = _raw(lib, call, h, 1, n, X, B, None, None, mm)[0]
                out[pre + "2"] = _raw(lib, call, h, 2, n, X, None, Z, None, mm)[0]
                out[pre + "3"] = _raw(lib, call, h, 3, n, X, B, None, dinv, mm)[0]
                out[pre + "5"] = _raw(lib, call, h, 5, n, X, B, Z, dinv, mm)[0]
                out[pre + "4_y"], out[pre + "4_z"] = _raw(lib, call, h, 4, n, None, B, np.zeros(n), dinv, mm)
                out[pre + "4_no_z"] = _raw(lib, call, h, 4, n, None, B, None, dinv, mm)[0]
            out["apply_with_companion"] = h.apply(X)   # 16-bit or offset-coded columns where the policy takes them
        h.destroy()
    finally:
        lib.GeneoSetSpmvKind(1)
        lib.GeneoSetKernelVariant(b"sell_offsets", 1)
        if span is not None:
            if old_span is None:
                del os.environ["GENEO_LP_SPAN_MAX"]
            else:
                os.environ["GENEO_LP_SPAN_MAX"] = old_span
    return a, (X, B, Z, dinv), out


def digests(out):
    return {k: hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest() for k, v in out.items()}


def scipy_products(a, inputs):
    """the FP64 algebra each output stands for (companion outputs: to single precision of the values only)"""
    X, B, Z, dinv = inputs
    d = dinv if X.ndim == 1 else dinv[:, None]
    ax = a @ X
    ref = {"0": ax, "1": B - ax, "2": Z + ax, "3": X + W * d * (B - ax), "5": W * d * (Z + B) + ax,
           "4_y": B - a @ (W * d * B), "4_z": W * d * B, "4_no_z": B - a @ (W * d * B)}
    return lambda key: ax if key.startswith("apply") else ref[key.replace("fused", "").replace("single", "")]
