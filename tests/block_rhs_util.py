"""Shared checks of the block entry points (-geneo_block_width 16 | 32: PCMatApply_GenEO, MatMatMult_GenEO,
KSPMatSolve_GenEO), run by tests/test_block_rhs_host.py on the host twin and by tests/test_gpu_block_rhs.py on the HIP
library.  Every check takes the bound library; nothing here falls back from one to the other.

Argument table of GeneoTestBlockPrimitive (I = iarg, P = parg: device pointers of the caller, except suboff):
  cheb_dir_block   I(nsub, flags, w)  P(suboff HOST, coef, Z, D, X, dscale | NULL, Out)   slabs: n x w row-major
  block_import     I(ld, n, m, w)     P(Xcm, Yrm)        column-major n x m (ld) -> slab, columns m .. w - 1 zero
  block_export     I(ld, n, m, w)     P(Xrm, Ycm)        slab -> the first m columns, n rows each
  block_coldot     I(n, w)            P(X, Y, out)       out: w doubles
  block_axpy_cols  I(n, w)            P(Y, X, c)         Y[:, j] = fl(Y[:, j] + fl(c[j] X[:, j]))
  block_xpby_cols  I(n, w)            P(P, Z, c)         P[:, j] = fl(Z[:, j] + fl(c[j] P[:, j]))
  chol_solve_block I(n, w)            P(L, LT, Y)        Y: n x w row-major
Returns the primitive's bool as 0 / 1; GeneoSetKernelVariant("block_fused", 0) runs the composed forms of core.cpp.

Bound of the block apply against the single-vector apply (PARITY_BOUND).  Under -dls1_amg_precision double the two paths
are the same operator and differ by summation order alone (SpMM against SpMV in the V-cycle and the residual, Gram against
zt_apply).  The largest per-column relative 2-norm difference over SRAS,1 / RAS,0 / ASM,H1 / ORAS,1, m = 5 and m = 33, was
measured on the host twin and on an MI355X (profiles/r07_block_rhs.md); the bound is 100 x the larger of the two, and never
looser than the project's apply-parity bar of 1e-9.  ASM,E1 (the effHybrid branch of the composition) was measured the
same way afterwards: 0 on the host twin, at most 3.8e-15 on the MI355X -- inside the worst of the four, so the bound holds
for it unchanged."""
import ctypes as C
import functools
import math

import numpy as np

import cases
from primitive_cases import SENTF, Buf, _call, rnd, same_bits

MEASURED_HOST = 1.2e-16      # host twin: 1.154e-16 (profiles/r07_block_rhs.md)
MEASURED_GPU = 4.4e-15       # MI355X: 4.329e-15
PARITY_BOUND = min(1e-9, 100.0 * max(MEASURED_HOST, MEASURED_GPU))

BASE = ["-geneo_tau", "0.2", "-geneo_cut", "4", "-ksp_type", "cg", "-ksp_rtol", "1e-10", "-ksp_initial_guess_nonzero", "0",
        "-dls1_ksp_type", "chebyshev", "-dls1_ksp_rtol", "1e-7"]
DOUBLE = ["-dls1_amg_precision", "double"]
LEVELS = ("SRAS,1", "RAS,0", "ASM,H1", "ASM,E1", "ORAS,1")
SUBS = (1, 1025, 197)        # as tests/test_gpu_cheb_local_solver.py: a one-row chunk, a chunk boundary with a one-row tail
N_K = sum(SUBS)              # 1223 rows: more than one tile and one workgroup of every kernel, no multiple of 64


def argv_for(lvl, w, extra=()):
    return ["-geneo_lvl", lvl, "-geneo_block_width", str(w)] + BASE + list(extra)


@functools.lru_cache(maxsize=None)
def grid(n):
    return cases.grid_case(n=n, parts=(2, 2, 2), overlap=2)


_pcs = {}


def get_pc(lib, n, argv):
    """One set-up per (library, case, options), shared by the checks of a session (release_pcs at its end)."""
    key = (id(lib), n, tuple(argv))
    if key not in _pcs:
        mesh, dec, a, b = grid(n)
        _pcs[key] = cases.run_pc(lib, mesh, dec, list(argv), b)
    return _pcs[key]


def release_pcs(lib=None):
    for k in [k for k in _pcs if lib is None or k[0] == id(lib)]:
        _pcs.pop(k).destroy()


def call(lib, name, I=(), P=()):
    ia = (C.c_int * max(1, len(I)))(*[int(v) for v in I])
    da = (C.c_double * 1)(0.0)
    pa = (C.c_void_p * max(1, len(P)))(*[(p if (p is None or isinstance(p, int)) else p.ptr) for p in P])
    rc = lib.GeneoTestBlockPrimitive(name.encode(), ia, da, pa)
    assert rc >= 0, "%s: rc %d (%s)" % (name, rc, lib.PCGenEOGetError(None).decode())
    return rc


class block_fused_off:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.GeneoSetKernelVariant(b"block_fused", 0) == 0

    def __exit__(self, *a):
        assert self.lib.GeneoSetKernelVariant(b"block_fused", 1) == 0


def shifted(lib, arr, shift):
    """device copy of arr that starts `shift` doubles into its buffer (shift = 1: 8-byte aligned only); (Buf, pointer)"""
    b = Buf(lib, np.concatenate([np.full(shift, SENTF), np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)]))
    return b, b.ptr + 8 * shift


def fetch(buf, shift, shape):
    full = buf.get()                    # checks both canaries
    assert same_bits(full[:shift], np.full(shift, SENTF)), "write in front of the block"
    return full[shift:].reshape(shape)


def relcols(a, b):
    """largest per-column relative 2-norm difference"""
    den = np.linalg.norm(b, axis=0)
    den[den == 0.0] = 1.0
    return float(np.max(np.linalg.norm(a - b, axis=0) / den))


# ---------------------------------------------------------------------------------------------- 1. options and errors
def check_options_and_errors(lib):
    from geneo4petsc_amd.pc import GenEOError, GenEOPC
    mesh, dec, a, b = grid(12)
    pc = GenEOPC(lib)
    assert pc.options()["block_width"] == 0
    assert "-geneo_block_width" in pc.usage()
    for bad in ("8", "-16", "33", "64", "x"):
        with np.testing.assert_raises(GenEOError):
            pc.set_option("-geneo_block_width", bad)
    assert pc.options()["block_width"] == 0
    pc.set_option("-geneo_block_width", "32")
    assert pc.options()["block_width"] == 32
    pc.destroy()
    # a width with the cg local solver: the set-up fails and names both options
    try:
        cases.run_pc(lib, mesh, dec, ["-geneo_lvl", "SRAS,1", "-geneo_block_width", "16"] + BASE[:4] + ["-dls1_ksp_type", "cg"], b)
        raise AssertionError("the set-up accepted -geneo_block_width with -dls1_ksp_type cg")
    except GenEOError as e:
        assert "-geneo_block_width" in str(e) and "-dls1_ksp_type" in str(e), str(e)
    X = np.random.default_rng(1).standard_normal((mesh.nbNode, 3))
    # block calls on a PC without a width
    pc0 = get_pc(lib, 12, ["-geneo_lvl", "SRAS,1"] + BASE)
    assert pc0.block_info()["width"] == 0
    for fn in (pc0.mat_apply, pc0.mat_mult, pc0.mat_solve):
        try:
            fn(X)
            raise AssertionError("a block call on a PC without -geneo_block_width went through")
        except GenEOError as e:
            assert "-geneo_block_width" in str(e), str(e)
    # ... and on one that is not set up
    pcn = GenEOPC(lib)
    pcn.set_from_options(argv_for("SRAS,1", 16))
    with np.testing.assert_raises(GenEOError):
        pcn.mat_apply(X)
    pcn.destroy()
    # bad shapes, and the Krylov options the block solve refuses
    pc = get_pc(lib, 12, argv_for("SRAS,1", 16, DOUBLE))
    n = mesh.nbNode
    from geneo4petsc_amd.pc import DeviceVector
    xd, yd = DeviceVector.from_host(lib, X.ravel(order="F")), DeviceVector(lib, 3 * n)
    assert lib.PCMatApply_GenEO(pc.h, xd.ptr, n - 1, yd.ptr, n, 3) != 0 and "leading dimension" in lib.PCGenEOGetError(pc.h).decode()
    assert lib.MatMatMult_GenEO(pc.h, xd.ptr, n, yd.ptr, n - 1, 3) != 0
    assert lib.PCMatApply_GenEO(pc.h, xd.ptr, n, yd.ptr, n, 0) != 0 and "column" in lib.PCGenEOGetError(pc.h).decode()
    assert lib.MatMatMult_GenEO(pc.h, xd.ptr, n, yd.ptr, n, -2) != 0
    for key, val, word in (("-ksp_type", "gmres", "-ksp_type"), ("-ksp_initial_guess_nonzero", "1", "-ksp_initial_guess_nonzero")):
        pc.set_option(key, val)
        try:
            pc.mat_solve(X)
            raise AssertionError("KSPMatSolve_GenEO accepted %s %s" % (key, val))
        except GenEOError as e:
            assert word in str(e), str(e)
        finally:
            pc.set_option(key, "cg" if key == "-ksp_type" else "0")
    # the width is read by the set-up: changing it afterwards changes nothing before the next one
    pc.set_option("-geneo_block_width", "32")
    assert pc.block_info()["width"] == 16
    pc.set_option("-geneo_block_width", "16")


# ---------------------------------------------------------------------------------------------- 2. the kernels alone
@functools.lru_cache(maxsize=None)
def _cheb_data(flags):
    rng = np.random.default_rng(50 + flags)
    coef = rng.random((len(SUBS), 2)) + 0.25
    coef[:, 1] *= -1.0 if flags & 1 else 1.0
    coef[2] = 0.0                                             # a subdomain whose table row is (0, 0)
    return coef, rng.standard_normal((N_K, 32)), rng.standard_normal((N_K, 32)), rng.standard_normal((N_K, 32)), rng.standard_normal(N_K)


_cheb_ref = {}


def cheb_dir_reference(lib, flags, with_dscale):
    """GeneoTestPrimitive("cheb_dir") on each of the 32 columns: (D, X, Out) with the columns side by side.  Computed once
    per (library, flags, dscale) and never written."""
    key = (id(lib), flags, with_dscale)
    if key not in _cheb_ref:
        coef, Z, D, X, ds = _cheb_data(flags)
        off = np.concatenate([[0], np.cumsum(SUBS)]).astype(np.int32)
        dc, dds = Buf(lib, coef.reshape(-1)), Buf(lib, ds)
        out = [np.empty((N_K, 32)) for _ in range(3)]
        for j in range(32):
            bz, bd, bx, bo = (Buf(lib, v) for v in (Z[:, j], D[:, j], X[:, j], np.full(N_K, SENTF)))
            assert _call(lib, "cheb_dir", I=[len(SUBS), flags], P=[off, dc, bz, bd, bx, dds if with_dscale else None, bo]) == 1
            for o, b in zip(out, (bd, bx, bo)):
                o[:, j] = b.get()
            for b in (bz, bd, bx, bo):
                b.free()
        _cheb_ref[key] = out
    return _cheb_ref[key]


def check_cheb_dir_block(lib, w, flags, with_dscale):
    coef, Z, D, X, ds = _cheb_data(flags)
    refD, refX, refO = cheb_dir_reference(lib, flags, with_dscale)
    off = np.concatenate([[0], np.cumsum(SUBS)]).astype(np.int32)
    for shift in (0, 1):
        bc, pc_ = shifted(lib, coef.reshape(-1), shift)
        bs, ps = shifted(lib, ds, shift)
        bz, pz = shifted(lib, Z[:, :w], shift)
        bd, pd = shifted(lib, D[:, :w], shift)
        bx, px = shifted(lib, X[:, :w], shift)
        bo, po = shifted(lib, np.full((N_K, w), SENTF), shift)
        assert call(lib, "cheb_dir_block", I=[len(SUBS), flags, w],
                    P=[off.ctypes.data, pc_, pz, pd, px, ps if with_dscale else None, po]) == 1
        gD, gX, gO = (fetch(b, shift, (N_K, w)) for b in (bd, bx, bo))
        assert same_bits(fetch(bz, shift, (N_K, w)), Z[:, :w]) and same_bits(fetch(bs, shift, (N_K,)), ds)
        for j in range(w):
            what = "column %d, w %d, flags %d, dscale %s, shift %d" % (j, w, flags, with_dscale, shift)
            assert same_bits(gD[:, j], refD[:, j]), "d: " + what
            assert same_bits(gX[:, j], refX[:, j]), "x: " + what
            assert same_bits(gO[:, j], refO[:, j]), "out: " + what       # (flags without bit 1: the sentinel, untouched)
        r0, r1 = off[2], off[3]
        assert np.all(gD[r0:r1] == 0.0)
        for b in (bc, bs, bz, bd, bx, bo):
            b.free()


def check_import_export(lib, w):
    rng = np.random.default_rng(60 + w)
    n, ld = N_K, N_K + 3
    for m in (1, 5, 16, 17, 32, 33):
        data = rng.standard_normal((n, m))
        cm = np.full((m, ld), SENTF)                   # column-major with leading dimension ld: row j of this array = column j
        cm[:, :n] = data.T
        for shift in (0, 1):
            bin_, pin = shifted(lib, cm, shift)
            tgt = np.full((m + 1, ld), SENTF)
            bout, pout = shifted(lib, tgt, shift)
            for j0 in range(0, m, w):                  # one slab at a time, as the entry points do
                ms = min(w, m - j0)
                bs, pslab = shifted(lib, np.full((n, w), SENTF), shift)
                assert call(lib, "block_import", I=[ld, n, ms, w], P=[pin + 8 * j0 * ld, pslab]) == 1
                slab = fetch(bs, shift, (n, w))
                assert same_bits(slab[:, :ms], data[:, j0:j0 + ms]), (m, j0, shift)
                assert np.all(slab[:, ms:] == 0.0) and not np.signbit(slab[:, ms:]).any(), "padding columns are not zero"
                assert call(lib, "block_export", I=[ld, n, ms, w], P=[pslab, pout + 8 * j0 * ld]) == 1
                bs.free()
            assert same_bits(fetch(bin_, shift, (m, ld)), cm), "import changed its input"
            got = fetch(bout, shift, (m + 1, ld))
            assert same_bits(got[:m, :n], data.T), (m, shift)
            assert same_bits(got[:m, n:], tgt[:m, n:]), "rows between n and ld written"
            assert same_bits(got[m], tgt[m]), "column m written"
            bin_.free()
            bout.free()


def check_coldot(lib, w):
    """1e-13 relative to math.fsum of the same products, on X . Y with entries of one sign and on X . X: sums without
    cancellation, where "relative to the value" is what a summation order can be held to (a mixed-sign sum may cancel to any
    size; its error stays proportional to sum |x_i y_i|)."""
    rng = np.random.default_rng(70 + w)
    for n in (1, N_K, 20000):                          # one row; several workgroups; more rows than one pass of a workgroup
        X, Y = rng.random((n, w)) + 0.5, rng.random((n, w)) + 0.5
        X[:, 1::2] *= -1.0                             # whole columns negative: every product of a column has one sign
        res = []
        for rep in range(2):
            shift = rep                                # the second call on buffers that are 8-byte aligned only
            bx, px = shifted(lib, X, shift)
            by, py = shifted(lib, Y, shift)
            bo, po = shifted(lib, np.full(w, SENTF), shift)
            for a, b_ in ((px, py), (px, px)):
                assert call(lib, "block_coldot", I=[n, w], P=[a, b_, po]) == 1
                res.append(fetch(bo, shift, (w,)))
            for b_ in (bx, by, bo):
                b_.free()
        assert same_bits(res[0], res[2]) and same_bits(res[1], res[3]), "block_coldot: two calls, two results"
        for got, (A, B) in zip(res[:2], ((X, Y), (X, X))):
            for j in range(w):
                ref = math.fsum((A[:, j] * B[:, j]).tolist())
                assert abs(got[j] - ref) <= 1e-13 * abs(ref), (n, w, j, got[j], ref)


def check_col_updates(lib, w):
    rng = np.random.default_rng(80 + w)
    n = N_K
    Y, X, c = rng.standard_normal((n, w)), rng.standard_normal((n, w)), rng.standard_normal(w)
    c[3] = 0.0                                         # a frozen column: exactly unchanged / exactly Z
    for shift in (0, 1):
        by, py = shifted(lib, Y, shift)
        bx, px = shifted(lib, X, shift)
        bc, pcf = shifted(lib, c, shift)
        assert call(lib, "block_axpy_cols", I=[n, w], P=[py, px, pcf]) == 1
        got = fetch(by, shift, (n, w))
        assert same_bits(got, Y + c[None, :] * X), "block_axpy_cols, shift %d" % shift
        assert same_bits(got[:, 3], Y[:, 3])
        bp, pp = shifted(lib, Y, shift)
        assert call(lib, "block_xpby_cols", I=[n, w], P=[pp, px, pcf]) == 1
        got = fetch(bp, shift, (n, w))
        assert same_bits(got, X + c[None, :] * Y), "block_xpby_cols, shift %d" % shift
        assert same_bits(fetch(bx, shift, (n, w)), X) and same_bits(fetch(bc, shift, (w,)), c)
        for b_ in (by, bx, bc, bp):
            b_.free()


@functools.lru_cache(maxsize=None)
def chol_case(n):
    """the matrices of primitive_cases.case_chol_solve: Q diag(linspace(1, 100, n)) Q^T; (L, L^T, 32 right-hand sides)"""
    rng = np.random.default_rng(1000 + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * np.linspace(1.0, 100.0, n)) @ q.T
    lo = np.linalg.cholesky(0.5 * (a + a.T))
    return lo, np.ascontiguousarray(lo.T), rnd(rng, n, 32)


_chol_ref = {}


def check_chol_solve_block(lib, w, n):
    """Per column the bits of the one-workgroup sweeps: bk::chol_solve, through GeneoTestPrimitive("chol_solve")."""
    lo, lt, rhs = chol_case(n)
    dl, dlt = Buf(lib, lo), Buf(lib, lt)
    key = (id(lib), n)
    if key not in _chol_ref:
        ref = np.empty((n, 32))
        for j in range(32):
            o = Buf(lib, rhs[:, j])
            assert _call(lib, "chol_solve", I=[n], P=[dl, dlt, o]) == 1
            ref[:, j] = o.get()
            o.free()
        _chol_ref[key] = ref
    ref = _chol_ref[key]
    by = Buf(lib, rhs[:, :w])
    assert call(lib, "chol_solve_block", I=[n, w], P=[dl, dlt, by]) == 1
    got = by.get()
    assert same_bits(dl.get(), lo) and same_bits(dlt.get(), lt)
    for j in range(w):
        assert same_bits(got[:, j], ref[:, j]), "chol_solve_block n %d w %d column %d" % (n, w, j)
    x = np.linalg.solve(lo @ lt, rhs[:, :w])
    assert np.linalg.norm(got - x) <= 1e-10 * np.linalg.norm(x)
    for b_ in (dl, dlt, by):
        b_.free()


# ---------------------------------------------------------------------------------------------- 3 .. 7: the entry points
def rhs_block(n, m, seed):
    return np.random.default_rng(seed).standard_normal((n, m))


def check_mat_mult(lib, n, w, m):
    pc = get_pc(lib, n, argv_for("SRAS,1", w, DOUBLE))
    X = rhs_block(grid(n)[0].nbNode, m, 11)
    Y = pc.mat_mult(X)
    ref = np.stack([pc.matmult(X[:, j]) for j in range(m)], axis=1)
    err = relcols(Y, ref)
    print("MatMatMult against MatMult, %d^3, w %d, m %d: %.3e" % (n, w, m, err))
    assert err <= 1e-13
    a = grid(n)[2]
    assert relcols(Y, a @ X) <= 1e-13


def measure_mat_apply(lib, n, w, lvl, m):
    """largest per-column relative difference of PCMatApply to PCApply on the same set-up (-dls1_amg_precision double)"""
    pc = get_pc(lib, n, argv_for(lvl, w, DOUBLE))
    X = rhs_block(grid(n)[0].nbNode, m, 12 + m)
    Y = pc.mat_apply(X)
    ref = np.stack([pc.apply(X[:, j]) for j in range(m)], axis=1)
    assert np.isfinite(Y).all()
    return relcols(Y, ref)


def check_mat_apply(lib, n, w, lvl, m):
    err = measure_mat_apply(lib, n, w, lvl, m)
    print("PCMatApply against PCApply, %d^3, %s, w %d, m %d: %.3e (bound %.1e)" % (n, lvl, w, m, err, PARITY_BOUND))
    assert err <= PARITY_BOUND
    return err


def check_column_independence(lib, n, w, lvl="SRAS,1"):
    pc = get_pc(lib, n, argv_for(lvl, w, DOUBLE))
    X = rhs_block(grid(n)[0].nbNode, 5, 13)
    Y = pc.mat_apply(X)
    for j in range(5):
        yj = pc.mat_apply(X[:, j:j + 1])
        assert same_bits(yj[:, 0], Y[:, j]), "%s: column %d of a 5-column apply differs from the apply of that column alone (%.3e)" % (
            lvl, j, np.linalg.norm(yj[:, 0] - Y[:, j]) / np.linalg.norm(Y[:, j]))


def check_symmetry(lib, n, w):
    """the default -dls1_amg_precision single: the block operator is another operator than the single-vector one there
    (FP64 level matrices against their float companions), but still fixed, linear and symmetric"""
    pc = get_pc(lib, n, argv_for("SRAS,1", w))
    X = rhs_block(grid(n)[0].nbNode, 5, 14)
    Y = pc.mat_apply(X)
    S = X.T @ Y
    asym = np.linalg.norm(S - S.T) / np.linalg.norm(S)
    Y2 = pc.mat_apply(X @ np.diag([2.0, -1.0, 0.5, 3.0, 1.0]))
    lin = relcols(Y2, Y @ np.diag([2.0, -1.0, 0.5, 3.0, 1.0]))
    single = np.stack([pc.apply(X[:, j]) for j in range(5)], axis=1)
    print("SRAS,1 default precision, %d^3: asymmetry of X^T M X %.3e, linearity %.3e, block against single-vector path %.3e"
          % (n, asym, lin, relcols(Y, single)))
    assert asym <= 1e-10
    assert lin <= 1e-13
    assert np.linalg.eigvalsh(0.5 * (S + S.T)).min() > 0.0


def solve_columns(n, seeds=(21, 22)):
    """A ones, two random columns, a zero column, a copy of column 1"""
    mesh, dec, a, b = grid(n)
    N = mesh.nbNode
    cols = [a @ np.ones(N), np.random.default_rng(seeds[0]).standard_normal(N), np.random.default_rng(seeds[1]).standard_normal(N),
            np.zeros(N)]
    cols.append(cols[1].copy())
    return np.stack(cols, axis=1)


SOLVE = DOUBLE + ["-els2_eps_tol", "1e-10"]     # eigenpairs converged: the coarse space, and with it the residual history of
                                                # a column, is then the same on every backend up to rounding


def check_mat_solve(lib, n, w, lvl="SRAS,1", seeds=(21, 22), B=None, singles=None):
    """seeds: picked on the host twin so that no column hovers at its threshold (the check below)"""
    pc = get_pc(lib, n, argv_for(lvl, w, SOLVE))
    mesh, dec, a, b = grid(n)
    B = solve_columns(n, seeds) if B is None else B
    m = B.shape[1]
    rtol = 1e-10
    if singles is None:
        singles = []
        for j in range(m):
            x, its, rnorm, reason = pc.solve(B[:, j], x0=np.zeros(mesh.nbNode))
            singles.append((x, its, reason, pc.residual_history().copy()))
    # the inputs first, on the single-vector histories alone: no column may hover at its threshold
    for j, (x, its, reason, hist) in enumerate(singles):
        if its == 0:
            continue
        thr = rtol * hist[0]
        assert hist[-1] < 0.95 * thr and hist[-2] > 1.05 * thr, \
            "bad input: column %d hovers at its threshold (%.3e, %.3e against %.3e): pick another seed" % (j, hist[-2], hist[-1], thr)
    assert len({s[1] for s in singles if s[1] > 0}) >= 2, "bad input: every column converges at the same iteration: freezing is not exercised"
    X, its, rnorm, reasons = pc.mat_solve(B)
    print("KSPMatSolve %s %d^3 w %d: its %s (single-vector %s)" % (lvl, n, w, list(its), [s[1] for s in singles]))
    for j, (x, sits, sreason, hist) in enumerate(singles):
        assert its[j] == sits and reasons[j] == sreason, (j, its[j], sits, reasons[j], sreason)
        if np.any(B[:, j]):
            assert np.linalg.norm(X[:, j] - x) <= 1e-10 * np.linalg.norm(x), (j, np.linalg.norm(X[:, j] - x) / np.linalg.norm(x))
            assert np.linalg.norm(B[:, j] - a @ X[:, j]) <= 1e-8 * np.linalg.norm(B[:, j])
            assert abs(rnorm[j] - hist[-1]) <= 1e-6 * hist[-1]
    assert its[3] == 0 and reasons[3].startswith("KSP_CONVERGED") and not np.any(X[:, 3])
    assert same_bits(X[:, 4], X[:, 1]) and its[4] == its[1] and rnorm[4] == rnorm[1]
    return X, its, reasons


def live_bytes(lib):
    """device bytes the library has handed out now (Python-side garbage collected first)"""
    import gc
    gc.collect()
    v = C.c_double(0.0)
    assert lib.GeneoDeviceMemInfo(C.byref(v), None, None, None, None, None, 0) == 0
    return v.value


def check_resetup(lib):
    """A second set-up followed by an apply gives the bits of the first, and after a set-up without a width behind one
    with a width the single-vector path gives the bits of a PC that never had one."""
    mesh, dec, a, b = grid(12)
    X = rhs_block(mesh.nbNode, 5, 17)
    plain = ["-geneo_lvl", "SRAS,1"] + BASE + DOUBLE
    fresh = get_pc(lib, 12, plain).apply(X[:, 0])
    pc = cases.run_pc(lib, mesh, dec, plain + ["-geneo_block_width", "32"], b)
    assert pc.block_info()["width"] == 32
    Y = pc.mat_apply(X)
    pc.setup(b)
    assert pc.block_info() == dict(width=32, slabs=0, columns=0, padded=0, graph_launches=0)
    assert same_bits(pc.mat_apply(X), Y)
    pc.set_option("-geneo_block_width", "0")
    pc.setup(b)
    assert pc.block_info()["width"] == 0
    assert same_bits(pc.apply(X[:, 0]), fresh)
    pc.destroy()


def memory_readings(lib):
    """Live device bytes of the library, relative to the reading before the first PC: after a fresh set-up without a width,
    after its destroy, after a set-up with width 32, after a set-up without a width behind it, after its destroy.
    Meant for a process of its own with GENEO_ALLOC_CACHE=0 (tests/block_mem_worker.py): the caching allocator may serve a
    request from a parked block up to an eighth larger and counts whole blocks, so with it the readings depend on what
    earlier work has parked; without it they are the bytes asked for."""
    from geneo4petsc_amd.pc import DeviceVector
    mesh, dec, a, b = grid(12)
    plain = ["-geneo_lvl", "SRAS,1"] + BASE + DOUBLE
    bdev = DeviceVector.from_host(lib, b)                    # one right-hand side on the device for every set-up
    empty = live_bytes(lib)
    out = {}
    pc = cases.run_pc(lib, mesh, dec, plain, bdev)
    out["fresh"] = live_bytes(lib) - empty
    pc.destroy()
    out["fresh_destroyed"] = live_bytes(lib) - empty
    pc = cases.run_pc(lib, mesh, dec, plain + ["-geneo_block_width", "32"], bdev)
    out["with_width"] = live_bytes(lib) - empty
    pc.mat_apply(rhs_block(mesh.nbNode, 5, 17))
    pc.set_option("-geneo_block_width", "0")
    pc.setup(bdev)
    out["width_removed"] = live_bytes(lib) - empty
    pc.destroy()
    out["destroyed"] = live_bytes(lib) - empty
    return out
