"""-m gpu: offset-coded columns of stencil slices (Csr::off_rec / off_mask, k_off_code, ColsOffset in backend_hip.hip).

In a coded 64-row slice every column is `row + one of at most 8 constants`; the FP64 SpMV (k_spmv_sell) and the passes over
the single-precision companion (k_spmv_sell_lp, every epilogue) then take their columns from one presence byte per row and
the slice's offsets instead of the 16-bit column stream.  Values, their order and the summation order are untouched, so the
path must agree TO THE BIT with the stored columns: every case runs both in one process (set_variant "sell_offsets" 1 / 0)
and compares with np.array_equal.  The shapes are the smallest at which the decode can go wrong: boundary rows with missing
entries in every slice, a ragged last slice, blocks with cut corner lines (per-slice fallback), plane offsets that need all
32 bits, an eighth offset, and matrices that must not be coded at all."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()          # raises if the HIP library is missing: no fallback


def _box(nx, ny, nz, rng, cut=False, points=7):
    """A box in natural order (x fastest) with random non-zero values on a 7- or 27-point pattern.  cut: the last two
    lines of every plane are 1 and 2 nodes short (the corner cut of an overlap-2 subdomain block)."""
    present = np.ones((nz, ny, nx), dtype=bool)
    if cut:
        present[:, ny - 2, nx - 1:] = False
        present[:, ny - 1, nx - 2:] = False
    idx = np.full(present.shape, -1, dtype=np.int64)
    idx[present] = np.arange(present.sum())
    if points == 7:
        nbrs = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    else:
        nbrs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    z, y, x = np.nonzero(present)
    rows, cols = [], []
    for dz, dy, dx in nbrs:
        zz, yy, xx = z + dz, y + dy, x + dx
        ok = (zz >= 0) & (zz < nz) & (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
        j = np.full(len(z), -1, dtype=np.int64)
        j[ok] = idx[zz[ok], yy[ok], xx[ok]]
        ok &= j >= 0
        rows.append(idx[z[ok], y[ok], x[ok]])
        cols.append(j[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (rng.random(len(rows)) + 0.5) * rng.choice([-1.0, 1.0], size=len(rows))
    n = int(present.sum())
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a.sort_indices()
    return a


def _pre_without_z(lib, h, B, dinv, w):
    """EPI_PRE with a null z (Spmv.fused_single always passes one)"""
    from geneo4petsc_amd.pc import DeviceVector
    bd, dd, yd = DeviceVector.from_host(lib, B), DeviceVector.from_host(lib, dinv), DeviceVector(lib, h.n)
    assert lib.GeneoSpmvFusedSingle(h.h, 4, None, yd.ptr, bd.ptr, None, dd.ptr, float(w)) == 0
    return yd.to_host()


def _on_off(lib, a, seed):
    """(slices, coded) and the outputs of every affected launch with the coded path on and off"""
    from geneo4petsc_amd.pc import Spmv
    n = a.shape[0]
    rng = np.random.default_rng(seed)
    X, B, Z = rng.random(n) + 0.25, rng.random(n) + 0.25, rng.random(n) - 0.5
    dinv, w = rng.random(n) + 0.5, 0.61
    h = Spmv(a, lib)
    h.fused_single(0, X=X)             # builds the companion and, with it, the offset coding
    info = h.offset_info()
    res = []
    try:
        for on in (1, 0):
            assert lib.GeneoSetKernelVariant(b"sell_offsets", on) == 0
            out = [h.apply(X), h.fused_single(0, X=X)[0], h.fused_single(1, X=X, B=B)[0], h.fused_single(2, X=X, Z=Z)[0],
                   h.fused_single(3, X=X, B=B, dinv=dinv, w=w)[0], h.fused_single(5, X=X, B=B, Z=Z, dinv=dinv, w=w)[0]]
            out += list(h.fused_single(4, B=B, dinv=dinv, w=w))
            out.append(_pre_without_z(lib, h, B, dinv, w))
            res.append(out)
    finally:
        lib.GeneoSetKernelVariant(b"sell_offsets", 1)
    h.destroy()
    names = ["apply", "NONE", "RES", "ADD", "JAC", "POST", "PRE y", "PRE z", "PRE without z"]
    for name, y1, y0 in zip(names, *res):
        assert np.array_equal(y1, y0), name
    # the FP64 product itself, against scipy: rows of at most 27 entries of magnitude <= 1.5 x 1.25
    np.testing.assert_allclose(res[0][0], a @ X, rtol=1e-12, atol=1e-12)
    return info


def test_box_7pt_every_slice_coded(lib):
    """9 x 7 x 5 (315 rows, 5 slices): boundary rows with missing entries in every slice, a ragged last slice"""
    a = _box(9, 7, 5, np.random.default_rng(1))
    assert a.shape[0] == 315
    slices, coded = _on_off(lib, a, 2)
    assert (slices, coded) == (5, 5)


def test_two_blocks_with_cut_corners_fall_back_slice_by_slice(lib):
    """9 x 7 x 5 followed by 6 x 11 x 4 with the last two lines of every plane 1 and 2 nodes short: the second block
    starts at row 315 (not a multiple of 64) and its slices see more than 8 offsets where they straddle the short lines"""
    rng = np.random.default_rng(3)
    a = sp.block_diag([_box(9, 7, 5, rng), _box(6, 11, 4, rng, cut=True)], format="csr")
    a.sort_indices()
    assert a.shape[0] == 315 + 4 * (6 * 11 - 3)
    slices, coded = _on_off(lib, a, 4)
    assert slices == (a.shape[0] + 63) // 64 == 9
    assert 0 < coded < slices
    # the pattern is fixed, and so is the count (the eligibility rule applied by hand to this matrix): 6 of 9 is under
    # 90 %, so this matrix keeps the stored-column kernels as a whole (the in-kernel fallback of single slices is the
    # next case)
    assert coded == 6 and 10 * coded < 9 * slices


def test_mostly_coded_matrix_runs_its_other_slices_on_the_stored_columns(lib):
    """30 x 10 x 10 followed by the cut 6 x 11 x 4 block: 47 of 51 slices coded, above the 90 % rule -- the coded kernels
    run, and the four slices over the short lines take the stored columns inside them"""
    rng = np.random.default_rng(13)
    a = sp.block_diag([_box(30, 10, 10, rng), _box(6, 11, 4, rng, cut=True)], format="csr")
    a.sort_indices()
    slices, coded = _on_off(lib, a, 14)
    assert (slices, coded) == (51, 47) and 10 * coded >= 9 * slices


def test_plane_offset_needs_32_bits(lib):
    """184 x 184 x 3 (101 568 rows): plane offset 33 856, a slice spans more than 65 535 columns (two column bases in the
    16-bit layout); the regime of the benchmark's 187^2 planes"""
    a = _box(184, 184, 3, np.random.default_rng(5))
    assert a.shape[0] == 101568
    slices, coded = _on_off(lib, a, 6)
    assert slices == 1587 and coded == slices


def test_large_matrix_takes_the_non_temporal_instantiations(lib):
    """84^3 (592 704 rows, 4.15 M stored entries): above both size thresholds of the non-temporal matrix stream (12 B x
    entries > 48 MB for the FP64 SpMV, 6 B x entries >= 24 MB for the companion passes), so the launches are the
    <.., NT = true, OFFS = true> instantiations the benchmark runs"""
    a = _box(84, 84, 84, np.random.default_rng(15))
    slices = (a.shape[0] + 63) // 64
    assert slices * 64 * 7 * 12 > 48e6 and slices * 64 * 7 * 6 >= 24e6
    assert _on_off(lib, a, 16) == (slices, slices)


def test_random_sparse_is_not_coded(lib):
    """300 rows, 5 random columns per row"""
    rng = np.random.default_rng(7)
    n = 300
    cols = np.concatenate([rng.choice(n, size=5, replace=False) for _ in range(n)])
    a = sp.csr_matrix((rng.random(5 * n) + 0.5, (np.repeat(np.arange(n), 5), cols)), shape=(n, n))
    a.sort_indices()
    slices, coded = _on_off(lib, a, 8)
    assert (slices, coded) == (5, 0)


def test_27pt_is_too_wide(lib):
    """6 x 6 x 6, 27-point: slices wider than 8 entries per row are not coded"""
    a = _box(6, 6, 6, np.random.default_rng(9), points=27)
    slices, coded = _on_off(lib, a, 10)
    assert (slices, coded) == (4, 0)


def test_explicit_zero_at_an_eighth_offset(lib):
    """the first case with one stored zero at column row + 3 of row 100: that slice has 8 offsets and stays coded"""
    a = _box(9, 7, 5, np.random.default_rng(1)).tocoo()
    assert not np.any((a.row == 100) & (a.col == 103))
    a = sp.csr_matrix((np.append(a.data, 0.0), (np.append(a.row, 100), np.append(a.col, 103))), shape=a.shape)
    a.sort_indices()
    assert a.nnz == _box(9, 7, 5, np.random.default_rng(1)).nnz + 1 and a[100].nnz == 8
    slices, coded = _on_off(lib, a, 11)
    assert (slices, coded) == (5, 5)


@pytest.mark.parametrize("parts", [(2, 2, 2), (2, 1, 1)])
def test_solve_is_unchanged(lib, parts):
    """20^3 in 8 subdomains at the benchmark's options: outer iterations, residual history, solution and the inner
    iteration count of the local solves are the same with the coded path on and off.  The 12^3-odd blocks of the 2 x 2 x 2
    split have cut corner lines in most of their slices and stay under the 90 % rule (the fine operators keep their stored
    columns, whatever the switch says); the two slabs of the 2 x 1 x 1 split are perfect boxes and run the coded kernels."""
    import cases
    mesh, dec, a, b = cases.grid_case(n=20, dim=3, parts=parts, overlap=2)
    res = []
    try:
        for on in (1, 0):
            assert lib.GeneoSetKernelVariant(b"sell_offsets", on) == 0
            pc = cases.run_pc(lib, mesh, dec, cases.bench_argv(), b)
            x, its, rnorm, reason = pc.solve(b)
            res.append((x, its, reason, np.array(pc.residual_history()), pc.info()["dls1_iterations"]))
            pc.destroy()
    finally:
        lib.GeneoSetKernelVariant(b"sell_offsets", 1)
    (x1, its1, r1, h1, inner1), (x0, its0, r0, h0, inner0) = res
    assert r1.startswith("KSP_CONVERGED") and r1 == r0
    assert its1 == its0
    assert np.array_equal(h1, h0)
    assert np.array_equal(x1, x0)
    assert inner1 == inner0
