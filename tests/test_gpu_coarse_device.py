"""-m gpu: the coarse operator E factored and solved on the device at any dimE (coarse_dev.hip; -geneo_coarse_device,
-geneo_coarse_block; GeneoTestCoarseFactor / GeneoTestCoarseSolve / PCGenEOGetCoarseInfo).

Bounds, with u = 2^-53 and gamma_k = k u / (1 - k u), references in numpy longdouble:
  * factorisation: |E - L L^T| <= gamma_{n+1} |L| |L^T| componentwise (Higham, Accuracy and Stability of Numerical
    Algorithms, theorem 10.3): it holds for every summation order and with fused multiply-adds as long as every entry of
    L comes from a substitution -- a panel multiplied by an inverted diagonal block would not meet it.  |L| |L^T| is
    evaluated in float64 (non-negative sums: relative error below n u, 1.5e-13 here) and shrunk by 1e-10, so the bar is
    never wider than the stated one.
  * sweeps: |L L^T x - b| <= (2 gamma_n + gamma_n^2) |L| |L^T| |x| componentwise: two substitutions, each backward stable
    with gamma_n in any order of its sums.
  * blocked sweeps against the one-workgroup kernel (n <= 1024): both solve (A + dA) x = b with |dA| below the bound
    above, A = Q diag(1 .. 100) Q^T, so || |L| |L^T| ||_2 <= ||L||_F^2 = trace(A) and lambda_min(A) = 1; to first order
    ||x1 - x2||_2 <= 2 (2 gamma_n + gamma_n^2) trace(A) ||x||_2 (taken with a factor 1.01 for the higher orders).
Shapes: every n / nb pair crosses a different edge -- one unknown, one short of / exactly / one past a block, several blocks
with a ragged last one (200 = 12.5 blocks of 16: three 64-row tiles of the trailing update and a ragged fourth), a single
ragged block one short of / exactly at / one past a wave, the old limit 1024 and
one past it, and 1300 = ten blocks of the default 128 plus 20."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
from cases import TIGHT

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
DEFAULT_NB = 128
SHAPES = [(n, 16) for n in (1, 15, 16, 17, 40, 200)] + [(n, DEFAULT_NB) for n in (63, 64, 65, 1024, 1025, 1300)]


def gamma(k):
    return k * U / (1.0 - k * U)


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()          # raises if the HIP library is missing: no fallback


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@functools.lru_cache(maxsize=None)
def spd(n, negate=False):
    """Q diag(linspace(1, 100, n)) Q^T, symmetrised (the matrices of primitive_cases.case_chol_solve); negate: the middle
    eigenvalue with the opposite sign.  Cached: shared by the tests and never written."""
    rng = np.random.default_rng(1000 + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.linspace(1.0, 100.0, n)
    if negate:
        d[n // 2] = -d[n // 2]
    a = (q * d) @ q.T
    a = np.ascontiguousarray(0.5 * (a + a.T))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def numpy_factor(n):
    lo = np.ascontiguousarray(np.linalg.cholesky(spd(n)))
    lt = np.ascontiguousarray(lo.T)
    b = np.random.default_rng(2000 + n).standard_normal(n)
    for v in (lo, lt, b):
        v.setflags(write=False)
    return lo, lt, b


def factor(lib, a, nb):
    n = a.shape[0]
    lo, lt = np.full((n, n), np.nan), np.full((n, n), np.nan)
    st = C.c_int(-1)
    rc = lib.GeneoTestCoarseFactor(n, nb, _p(a), _p(lo), _p(lt), C.byref(st))
    assert rc == 0, "GeneoTestCoarseFactor: %d %s" % (rc, lib.PCGenEOGetError(None).decode())
    return lo, lt, st.value


def solve(lib, lo, lt, b, nb, reps=1):
    y = b.copy()
    rc = lib.GeneoTestCoarseSolve(lo.shape[0], nb, _p(lo), _p(lt), _p(y), reps)
    assert rc == 0, "GeneoTestCoarseSolve: %d %s" % (rc, lib.PCGenEOGetError(None).decode())
    return y


def lower_products_ld(lo, blk=256):
    """the lower triangle of L L^T in longdouble, block by block over the columns that are not structurally zero"""
    n = lo.shape[0]
    ll = lo.astype(LD)
    out = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, blk):
        i1 = min(n, i0 + blk)
        for j0 in range(0, i1, blk):
            j1 = min(n, j0 + blk)
            out[i0:i1, j0:j1] = ll[i0:i1, :j1] @ ll[j0:j1, :j1].T
    return out


@pytest.mark.parametrize("n,nb", SHAPES)
def test_factorisation(lib, n, nb):
    a = spd(n)
    lo, lt, st = factor(lib, a, nb)
    assert st == 0
    assert not np.isnan(lo).any() and not np.isnan(lt).any()
    assert np.array_equal(np.triu(lo, 1).view(np.uint64), np.zeros((n, n), dtype=np.uint64)), "strict upper part of L"
    assert np.array_equal(lt.view(np.uint64), np.ascontiguousarray(lo.T).view(np.uint64)), "LT is not the transpose of L"
    low = np.tril(np.ones((n, n), dtype=bool))
    resid = np.abs(a.astype(LD) - lower_products_ld(lo))
    bound = gamma(n + 1) * (1.0 - 1e-10) * (np.abs(lo) @ np.abs(lo).T)
    ratio = float((resid[low] / bound[low]).max())
    print("factor n=%d nb=%d: |E - L L^T| at most %.3e of the bound" % (n, nb, ratio))
    assert (resid[low] <= bound[low]).all(), "n=%d nb=%d: %.3e of the bound" % (n, nb, ratio)
    lo2, lt2, st2 = factor(lib, a, nb)
    assert st2 == 0
    assert np.array_equal(lo.view(np.uint64), lo2.view(np.uint64)) and np.array_equal(lt.view(np.uint64), lt2.view(np.uint64))


@pytest.mark.parametrize("n,nb", [(40, 16), (1300, DEFAULT_NB)])
def test_not_positive_definite(lib, n, nb):
    """one negative eigenvalue: a non-zero status that names a pivot, and the call comes back (the hook reads every
    output: a kernel fault would surface as its error)"""
    lo, lt, st = factor(lib, spd(n, negate=True), nb)
    assert 0 < st <= n


@pytest.mark.parametrize("n,nb", SHAPES)
def test_sweeps(lib, n, nb):
    lo, lt, b = numpy_factor(n)
    x = solve(lib, lo, lt, b, nb)
    ll = lo.astype(LD)
    al = np.abs(ll)
    coef = 2 * gamma(n) + gamma(n) ** 2

    def check(v, what):
        resid = np.abs(ll @ (ll.T @ v.astype(LD)) - b)
        bound = coef * (al @ (al.T @ np.abs(v).astype(LD)))
        ratio = float((resid / bound).max())
        print("%s n=%d nb=%d: backward error %.3e of the bound" % (what, n, nb, ratio))
        assert (resid <= bound).all(), "%s n=%d nb=%d: backward error %.3e of the bound" % (what, n, nb, ratio)

    check(x, "blocked sweeps")
    x2 = solve(lib, lo, lt, b, nb)
    assert np.array_equal(x.view(np.uint64), x2.view(np.uint64)), "not reproducible"
    assert np.array_equal(solve(lib, lo, lt, b, nb, reps=3).view(np.uint64), x.view(np.uint64)), "repetitions differ"
    if n <= 1024:
        from primitive_cases import Buf, _call
        dl, dlt, o = Buf(lib, lo), Buf(lib, lt), Buf(lib, b)
        assert _call(lib, "chol_solve", I=[n], P=[dl, dlt, o]) == 1
        xc = o.get()
        check(xc, "chol_solve")
        bar = 1.01 * 2 * coef * float(np.trace(spd(n))) * np.linalg.norm(x)
        assert np.linalg.norm(x - xc) <= bar, (np.linalg.norm(x - xc), bar)


def test_host_reference_path_of_the_hooks(lib):
    """nb = 0: the host code the PC runs without the device kernels, through the same hooks (what scripts/coarse_bench.py
    times against the device); its factor meets the same bound and the blocked sweeps accept it"""
    n = 200
    a = spd(n)
    lo, lt, st = factor(lib, a, 0)
    assert st == 0 and np.array_equal(lt, lo.T) and not np.triu(lo, 1).any()
    low = np.tril(np.ones((n, n), dtype=bool))
    resid = np.abs(a.astype(LD) - lower_products_ld(lo))
    bound = gamma(n + 1) * (1.0 - 1e-10) * (np.abs(lo) @ np.abs(lo).T)
    assert (resid[low] <= bound[low]).all()
    b = numpy_factor(n)[2]
    xh, xd = solve(lib, lo, lt, b, 0), solve(lib, lo, lt, b, 16)
    assert np.linalg.norm(xh - xd) <= 1.01 * 2 * (2 * gamma(n) + gamma(n) ** 2) * float(np.trace(a)) * np.linalg.norm(xh)
    ms = (C.c_double(-2.0), C.c_double(-2.0))
    assert lib.GeneoTestCoarseElapsed(C.byref(ms[0]), C.byref(ms[1])) == 0
    assert ms[0].value >= 0.0 and ms[1].value >= 0.0


def test_bad_block_size_is_an_error(lib):
    a = spd(16)
    lo, lt = np.zeros((16, 16)), np.zeros((16, 16))
    st = C.c_int(0)
    assert lib.GeneoTestCoarseFactor(16, 24, _p(a), _p(lo), _p(lt), C.byref(st)) == -1
    assert "multiple of 16" in lib.PCGenEOGetError(None).decode()


def test_pc_forced_small(lib):
    """12^3 in 8 subdomains, 39 vectors each: dimE = 312 = 19 blocks of 16 and one of 8, through the whole PC"""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.9", "-geneo_cut", "39", "-ksp_type", "gmres"] + TIGHT + \
        ["-geneo_coarse_device", "always", "-geneo_coarse_block", "16"]
    _, info = cases.compare_with_oracle(lib, 12, (2, 2, 2), 1, argv)
    assert info["dimE"] == 312
    mesh, dec, a, b = cases.grid_case(n=12, parts=(2, 2, 2), overlap=1)
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    assert pc.coarse_info() == (312, 1, 2, 16)
    pc.destroy()


def test_pc_above_the_old_limit(lib):
    """16^3 in 8 subdomains, no cut: dimE = 1256.  Default options: device factor, blocked sweeps; never: the host's"""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.6", "-ksp_type", "gmres"] + TIGHT
    mesh, dec, a, b = cases.grid_case(n=16, parts=(2, 2, 2), overlap=1)
    res = []
    for extra in ([], ["-geneo_coarse_device", "never"]):
        pc = cases.run_pc(lib, mesh, dec, argv + extra, b)
        ci = pc.coarse_info()
        q = pc.apply_q(b)
        x, its, rnorm, reason = pc.solve(b)
        assert reason.startswith("KSP_CONVERGED")
        res.append((ci, q, its))
        pc.destroy()
    (ci_dev, q_dev, its_dev), (ci_never, q_never, its_never) = res
    assert ci_dev[1:] == (1, 2, DEFAULT_NB)
    assert ci_never[1:3] == (0, 0)
    assert ci_dev[0] == ci_never[0] == 1256
    assert its_dev == its_never
    rel = np.linalg.norm(q_dev - q_never) / np.linalg.norm(q_never)
    print("apply_q, device against never: %.3e" % rel)
    assert rel <= 2e-9
