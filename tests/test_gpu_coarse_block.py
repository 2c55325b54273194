"""-m gpu: the blocked coarse sweeps on blocks of right-hand sides (coarse_dev.hip: bk::coarse_solve_block;
GeneoTestCoarseSolveBlock, PCGenEOGetCoarseBlockCounters), HIP library, no fallback.

Kernel level: the matrices, numpy factors and shapes of tests/test_gpu_coarse_device.py (restated), each with w = 16 and 32
and a fixed-seed random n x w block.  Bounds, with u = 2^-53 and gamma_k = k u / (1 - k u), references in longdouble:
  * per column |L L^T x - b| <= (2 gamma_n + gamma_n^2) |L| |L^T| |x| componentwise: two substitutions, each backward stable
    with gamma_n in any order of its sums and with fused multiply-adds -- the bound of test_sweeps there;
  * against the single-vector sweeps (GeneoTestCoarseSolve on the column): both solve (A + dA) x = b with |dA| below that
    bound, A = Q diag(1 .. 100) Q^T, lambda_min(A) = 1, || |L| |L^T| ||_2 <= trace(A): to first order
    ||x_block - x_single||_2 <= 2 (2 gamma_n + gamma_n^2) trace(A) ||x||_2, taken with 1.01 for the higher orders.
Bits: the same input gives the same bits; a column's bits depend neither on its position in the block, nor on its
neighbours, nor on w; a zero column stays +0; L and L^T are not written (the hook compares them with what it uploaded and
keeps every buffer between canaries).

PC level: 12^3 in 2 x 2 x 2 subdomains at overlap 1 with tau 0.9 / cut 39 (dimE 312 = 19 blocks of 16 and one of 8), the
options of tests/block_rhs_util.py plus -geneo_coarse_device always -geneo_coarse_block 16, and one case above the old limit
(16^3, tau 0.6, dimE 1256, the default block 128).  PARITY: the largest per-column relative 2-norm difference of PCMatApply
to PCApply on the same PC and to PCMatApply under "block_fused" 0 (the column-by-column path: the parent's code) over
SRAS,1 / RAS,0 / ASM,E1, m = 5 and 33, w = 16 and 32 was measured once on an MI355X (profiles/r08_coarse_block.md); the
bound is 100 x that and never looser than the project's apply-parity bar of 1e-9."""
import ctypes as C
import functools

import numpy as np
import pytest

import block_rhs_util as U
import cases
from primitive_cases import same_bits

pytestmark = pytest.mark.gpu

UR = 2.0 ** -53
LD = np.longdouble
DEFAULT_NB = 128
SHAPES = [(n, 16) for n in (1, 15, 16, 17, 40, 200)] + [(n, DEFAULT_NB) for n in (63, 64, 65, 1024, 1025, 1300)]

MEASURED_PARITY = 3.4e-15    # MI355X: 3.368e-15 to PCApply (ASM,E1, m = 5), 2.184e-15 to the column-by-column path (SRAS,1, m = 33)
PARITY = min(1e-9, 100.0 * MEASURED_PARITY)

COARSE = ["-geneo_coarse_device", "always", "-geneo_coarse_block", "16"]
BASE = ["-geneo_tau", "0.9", "-geneo_cut", "39"] + U.BASE[4:]
LEVELS = ("SRAS,1", "RAS,0", "ASM,E1")


def gamma(k):
    return k * UR / (1.0 - k * UR)


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    lib = _lib.load()          # raises if the HIP library is missing: no fallback
    yield lib
    for k in list(_pcs):
        _pcs.pop(k).destroy()


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---------------------------------------------------------------------------------------------- kernel level
@functools.lru_cache(maxsize=None)
def spd(n):
    """Q diag(linspace(1, 100, n)) Q^T, symmetrised: the matrices of tests/test_gpu_coarse_device.py"""
    rng = np.random.default_rng(1000 + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * np.linspace(1.0, 100.0, n)) @ q.T
    a = np.ascontiguousarray(0.5 * (a + a.T))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def numpy_factor(n):
    """(L, L^T, B): the numpy factor of spd(n) and a fixed-seed n x 32 block (w = 16 takes its first 16 columns)"""
    lo = np.ascontiguousarray(np.linalg.cholesky(spd(n)))
    lt = np.ascontiguousarray(lo.T)
    B = np.ascontiguousarray(np.random.default_rng(3000 + n).standard_normal((n, 32)))
    for v in (lo, lt, B):
        v.setflags(write=False)
    return lo, lt, B


def solve_block(lib, lo, lt, B, nb, reps=1):
    """rc 0 also says: no canary broken, L and L^T and the input copy of Y unchanged (the hook compares them)"""
    n, w = B.shape
    y = np.ascontiguousarray(B).copy()
    rc = lib.GeneoTestCoarseSolveBlock(n, nb, w, _p(lo), _p(lt), _p(y), reps)
    assert rc == 0, "GeneoTestCoarseSolveBlock: %d %s" % (rc, lib.PCGenEOGetError(None).decode())
    return y


_blocks = {}


def block_solution(lib, n, nb, w):
    """the block solve of the first w columns of B: computed once per (n, nb, w), never written"""
    key = (id(lib), n, nb, w)
    if key not in _blocks:
        lo, lt, B = numpy_factor(n)
        x = solve_block(lib, lo, lt, B[:, :w], nb)
        x.setflags(write=False)
        _blocks[key] = x
    return _blocks[key]


_singles = {}


def single_solutions(lib, n, nb):
    """bk::coarse_solve on each of the 32 columns (the single-vector sweeps, unchanged): once per (n, nb)"""
    key = (id(lib), n, nb)
    if key not in _singles:
        lo, lt, B = numpy_factor(n)
        out = np.empty((n, 32))
        for j in range(32):
            y = np.ascontiguousarray(B[:, j]).copy()
            rc = lib.GeneoTestCoarseSolve(n, nb, _p(lo), _p(lt), _p(y), 1)
            assert rc == 0, "GeneoTestCoarseSolve: %d %s" % (rc, lib.PCGenEOGetError(None).decode())
            out[:, j] = y
        out.setflags(write=False)
        _singles[key] = out
    return _singles[key]


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_backward_error_per_column(lib, n, nb, w):
    lo, lt, B = numpy_factor(n)
    x = block_solution(lib, n, nb, w)
    assert np.isfinite(x).all()
    ll = lo.astype(LD)
    al = np.abs(ll)
    coef = 2 * gamma(n) + gamma(n) ** 2
    resid = np.abs(ll @ (ll.T @ x.astype(LD)) - B[:, :w])
    bound = coef * (al @ (al.T @ np.abs(x).astype(LD)))
    ratio = (resid / bound).max(axis=0)
    print("block sweeps n=%d nb=%d w=%d: backward error at most %.3e of the bound (column %d)"
          % (n, nb, w, float(ratio.max()), int(ratio.argmax())))
    assert (resid <= bound).all(), "n=%d nb=%d w=%d: %.3e of the bound" % (n, nb, w, float(ratio.max()))


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_agreement_with_the_single_vector_sweeps(lib, n, nb, w):
    x = block_solution(lib, n, nb, w)
    xs = single_solutions(lib, n, nb)[:, :w]
    coef = 2 * gamma(n) + gamma(n) ** 2
    bar = 1.01 * 2 * coef * float(np.trace(spd(n))) * np.linalg.norm(x, axis=0)
    diff = np.linalg.norm(x - xs, axis=0)
    print("block against single-vector sweeps n=%d nb=%d w=%d: at most %.3e of the bound" % (n, nb, w, float((diff / bar).max())))
    assert (diff <= bar).all(), (n, nb, w, float((diff / bar).max()))


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_reproducible(lib, n, nb, w):
    lo, lt, B = numpy_factor(n)
    x = block_solution(lib, n, nb, w)
    assert same_bits(solve_block(lib, lo, lt, B[:, :w], nb), x), "two calls, two results"
    assert same_bits(solve_block(lib, lo, lt, B[:, :w], nb, reps=3), x), "repetitions differ"


@pytest.mark.parametrize("n,nb", SHAPES)
def test_column_independence(lib, n, nb):
    """column 3 of the block: alone between zero columns, at another position (of either width), and at the other width"""
    lo, lt, B = numpy_factor(n)
    x16, x32 = block_solution(lib, n, nb, 16), block_solution(lib, n, nb, 32)
    for j in range(16):
        assert same_bits(x32[:, j], x16[:, j]), "column %d differs between w = 16 and w = 32" % j
    for w, x, pos in ((16, x16, 3), (16, x16, 12), (32, x32, 3), (32, x32, 29)):
        Z = np.zeros((n, w))
        Z[:, pos] = B[:, 3]
        z = solve_block(lib, lo, lt, Z, nb)
        assert same_bits(z[:, pos], x[:, 3]), "w %d: column 3 solved alone at position %d differs" % (w, pos)
        others = np.delete(z, pos, axis=1)
        assert not others.any() and not np.signbit(others).any(), "w %d: a zero column did not stay +0" % w


@pytest.mark.parametrize("w", [16, 32])
def test_zero_block_stays_zero(lib, w):
    lo, lt, B = numpy_factor(200)
    z = solve_block(lib, lo, lt, np.zeros((200, w)), 16)
    assert not z.any() and not np.signbit(z).any()


def test_bad_arguments_are_errors(lib):
    lo, lt, B = numpy_factor(16)
    for nb, w, word in ((16, 8, "16 or 32"), (24, 16, "multiple of 16")):
        y = np.ascontiguousarray(B[:, :w]).copy()
        assert lib.GeneoTestCoarseSolveBlock(16, nb, w, _p(lo), _p(lt), _p(y), 1) == -1
        assert word in lib.PCGenEOGetError(None).decode(), lib.PCGenEOGetError(None).decode()
        assert same_bits(y, B[:, :w])


# ---------------------------------------------------------------------------------------------- PC level
@functools.lru_cache(maxsize=None)
def grid(n):
    return cases.grid_case(n=n, parts=(2, 2, 2), overlap=1)


def argv_for(lvl, w, extra=()):
    return ["-geneo_lvl", lvl, "-geneo_block_width", str(w)] + BASE + U.DOUBLE + COARSE + list(extra)


_pcs = {}


def get_pc(lib, lvl, w, extra=()):
    """one set-up per (level, width, options), shared by the tests of this file"""
    key = (lvl, w, tuple(extra))
    if key not in _pcs:
        mesh, dec, a, b = grid(12)
        pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, w, extra), b)
        dimE = pc.coarse_info()[0]
        if lvl.endswith(",0"):                               # one level: no coarse space, nothing for the sweeps to do
            assert dimE == 0
        else:
            assert dimE > 32 and dimE % 16 != 0, dimE        # several block rows and a ragged last one
            assert pc.coarse_info() == (dimE, 1, 2, 16)      # device factor, blocked sweeps, block 16
        _pcs[key] = pc
    return _pcs[key]


def measure_mat_apply(lib, lvl, w, m):
    """(to PCApply on the same PC, to PCMatApply column by column -- "block_fused" 0, the parent's path)"""
    pc = get_pc(lib, lvl, w)
    X = U.rhs_block(grid(12)[0].nbNode, m, 40 + m)
    before = pc.coarse_block_counters()
    Y = pc.mat_apply(X)
    slabs = -(-m // w) if pc.coarse_info()[0] else 0         # (RAS,0 has no coarse space: its slabs never get here)
    mid = pc.coarse_block_counters()
    assert mid == dict(blocked=before["blocked"] + slabs, by_column=before["by_column"], host_blocks=0), (before, mid)
    assert np.isfinite(Y).all()
    ref = np.stack([pc.apply(X[:, j]) for j in range(m)], axis=1)
    with U.block_fused_off(lib):
        Yc = pc.mat_apply(X)
    after = pc.coarse_block_counters()
    assert after == dict(blocked=mid["blocked"], by_column=mid["by_column"] + slabs, host_blocks=0), (mid, after)
    return U.relcols(Y, ref), U.relcols(Y, Yc)


def test_coarse_info_reports_the_device_factor(lib):
    assert get_pc(lib, "SRAS,1", 16).coarse_info()[1:] == (1, 2, 16)


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("lvl", LEVELS)
@pytest.mark.parametrize("m", [5, 33])
def test_mat_apply(lib, w, lvl, m):
    to_apply, to_columns = measure_mat_apply(lib, lvl, w, m)
    print("PCMatApply %s w %d m %d: %.3e to PCApply, %.3e to the column-by-column path (bound %.1e)"
          % (lvl, w, m, to_apply, to_columns, PARITY))
    assert to_apply <= PARITY
    assert to_columns <= PARITY


def test_counters(lib):
    mesh, dec, a, b = grid(12)
    pc = cases.run_pc(lib, mesh, dec, argv_for("SRAS,1", 16), b)
    zero = dict(blocked=0, by_column=0, host_blocks=0)
    assert pc.coarse_block_counters() == zero
    X = U.rhs_block(mesh.nbNode, 33, 41)
    pc.mat_apply(X)                                          # 3 slabs
    pc.mat_apply(X[:, :5])                                   # 1 slab
    assert pc.coarse_block_counters() == dict(blocked=4, by_column=0, host_blocks=0)
    pc.apply(X[:, 0])                                        # the single-vector path counts nothing
    assert pc.coarse_block_counters() == dict(blocked=4, by_column=0, host_blocks=0)
    with U.block_fused_off(lib):
        pc.mat_apply(X)
    assert pc.coarse_block_counters() == dict(blocked=4, by_column=3, host_blocks=0)
    info = pc.block_info()
    assert info["slabs"] == 7
    pc.setup(b)
    assert pc.coarse_block_counters() == zero
    pc.destroy()


@pytest.mark.parametrize("w", [16, 32])
def test_column_independence_through_the_pc(lib, w):
    pc = get_pc(lib, "SRAS,1", w)
    X = U.rhs_block(grid(12)[0].nbNode, 5, 42)
    Y = pc.mat_apply(X)
    for j in range(5):
        yj = pc.mat_apply(X[:, j:j + 1])
        assert same_bits(yj[:, 0], Y[:, j]), "column %d of a 5-column apply differs from the apply of that column alone (%.3e)" % (
            j, np.linalg.norm(yj[:, 0] - Y[:, j]) / np.linalg.norm(Y[:, j]))


SOLVE_SEEDS = (21, 22)


@pytest.mark.parametrize("w", [16, 32])
def test_mat_solve_equals_solve_column_by_column(lib, w):
    """the five columns of block_rhs_util.solve_columns: per column the iteration count and the reason of the
    single-vector solve from a zero guess, and its solution to 1e-10"""
    pc = get_pc(lib, "ASM,1", w, ("-els2_eps_tol", "1e-10"))
    mesh, dec, a, b = grid(12)
    B = U.solve_columns(12, SOLVE_SEEDS)
    rtol = 1e-10
    singles = []
    for j in range(B.shape[1]):
        x, its, rnorm, reason = pc.solve(B[:, j], x0=np.zeros(mesh.nbNode))
        singles.append((x, its, reason, pc.residual_history().copy()))
    for j, (x, its, reason, hist) in enumerate(singles):      # the inputs first: no column may hover at its threshold
        if its == 0:
            continue
        thr = rtol * hist[0]
        assert hist[-1] < 0.95 * thr and hist[-2] > 1.05 * thr, \
            "bad input: column %d hovers at its threshold (%.3e, %.3e against %.3e): pick another seed" % (j, hist[-2], hist[-1], thr)
    before = pc.coarse_block_counters()
    X, its, rnorm, reasons = pc.mat_solve(B)
    after = pc.coarse_block_counters()
    print("KSPMatSolve ASM,1 12^3 w %d: its %s (single-vector %s)" % (w, list(its), [s[1] for s in singles]))
    assert after["blocked"] > before["blocked"] and after["by_column"] == before["by_column"] and after["host_blocks"] == 0
    for j, (x, sits, sreason, hist) in enumerate(singles):
        assert its[j] == sits and reasons[j] == sreason, (j, its[j], sits, reasons[j], sreason)
        if np.any(B[:, j]):
            assert np.linalg.norm(X[:, j] - x) <= 1e-10 * np.linalg.norm(x), (j, np.linalg.norm(X[:, j] - x) / np.linalg.norm(x))
    assert its[3] == 0 and not np.any(X[:, 3])
    assert same_bits(X[:, 4], X[:, 1]) and its[4] == its[1]


def test_above_the_old_limit(lib):
    """16^3 in 8 subdomains, tau 0.6, no cut, default -geneo_coarse_device auto: dimE = 1256 = 9 blocks of 128 and one of 104"""
    mesh, dec, a, b = grid(16)
    argv = ["-geneo_lvl", "SRAS,1", "-geneo_block_width", "32", "-geneo_tau", "0.6"] + U.BASE[4:] + U.DOUBLE
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    dimE = pc.coarse_info()[0]
    assert dimE > 1024 and pc.coarse_info() == (dimE, 1, 2, DEFAULT_NB)
    X = U.rhs_block(mesh.nbNode, 5, 43)
    Y = pc.mat_apply(X)
    assert pc.coarse_block_counters() == dict(blocked=1, by_column=0, host_blocks=0)
    ref = np.stack([pc.apply(X[:, j]) for j in range(5)], axis=1)
    err = U.relcols(Y, ref)
    print("PCMatApply against PCApply, 16^3, dimE %d, w 32: %.3e (bound %.1e)" % (dimE, err, PARITY))
    assert err <= PARITY
    pc.destroy()
