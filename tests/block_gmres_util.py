"""Shared checks of the block GMRES of KSPMatSolve_GenEO (-ksp_matsolve_type gmres) and of its Gram-Schmidt primitives, run
by tests/test_block_gmres_host.py on the host twin and by tests/test_gpu_block_gmres.py on the HIP library.  Every check
takes the bound library; nothing here falls back from one to the other.

Argument table of GeneoTestBlockPrimitive for the primitives of this change (I = iarg, P = parg: device pointers):
  block_gs_dots    I(nb, n, w)  P(V table, W, H, work)               H: nb x w; work: nwg(n) x nb x w doubles
  block_gs_update  I(nb, n, w)  P(Y, V table, C, norm2 | NULL, work | NULL)   C: nb x w; norm2: w; work: 1024 x w
  block_scale_cols I(n, w)      P(Out, X, c)                         Out may be X
  block_gs_group   -                                                 returns the group size G of block_gs_dots
The V table is an array of nb slab pointers ON THE DEVICE.  GeneoSetKernelVariant("block_fused", 0) runs the composed
forms of core.cpp (one block_coldot / block_axpy_cols per slab).

Bound of the block solve against the single-vector solve (PARITY_BOUND).  Under -dls1_amg_precision double the two
preconditioners differ by summation order alone, and so do the two Gram-Schmidt processes; both solves stop at the same
iteration (the inputs are checked for that first), so their solutions differ by rounding amplified through the Krylov
recurrences.  The largest per-column relative 2-norm difference over the cases of CASES, with the default restart and with
-ksp_gmres_restart 5, was measured on the host twin and on an MI355X (profiles/r09_block_gmres.md); the bound is 100 x the
larger of the two, and never looser than 1e-7."""
import ctypes as C
import functools

import numpy as np

import block_rhs_util as U
import cases
from primitive_cases import SENTF, Buf, same_bits

MEASURED_HOST = 7.3e-15     # host twin: 7.232e-15 (profiles/r09_block_gmres.md)
MEASURED_GPU = 1.2e-10      # MI355X: 1.191e-10 (SRAS,1 with the default restart: 43 - 45 iterations, two cycles of classical
                             # Gram-Schmidt; every other case stays below 2.9e-14)
PARITY_BOUND = min(1e-7, 100.0 * max(MEASURED_HOST, MEASURED_GPU))

GMRES = ["-ksp_type", "gmres", "-ksp_matsolve_type", "gmres"]
# (level, grid, width, the seeds of the two random columns): seeds picked on the host twin so that no column hovers at its
# threshold, with the default restart and with -ksp_gmres_restart 5, and so that with -ksp_gmres_restart 5 the two random
# columns stop in different cycles, one of them in the middle of its cycle
CASES = (("RAS,1", 12, 16, (26, 30)), ("RAS,1", 20, 32, (22, 29)), ("ORAS,1", 12, 16, (26, 30)), ("SRAS,1", 12, 16, (44, 39)))
RESTART5 = ["-ksp_gmres_restart", "5"]
COLDOT_WG = 1024


def nwg(n):
    return max(1, min(COLDOT_WG, (n + 63) // 64))


def gs_group(lib):
    ia, da, pa = (C.c_int * 1)(0), (C.c_double * 1)(0.0), (C.c_void_p * 1)(None)
    g = lib.GeneoTestBlockPrimitive(b"block_gs_group", ia, da, pa)
    assert g >= 1, "block_gs_group: rc %d" % g
    return g


def argv_for(lvl, w, extra=()):
    return U.argv_for(lvl, w, U.SOLVE + GMRES + list(extra))


# ---------------------------------------------------------------------------------------------- the primitives alone
@functools.lru_cache(maxsize=4)
def _slabs(n, w, nb, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, w)) for _ in range(nb)], rng.standard_normal((n, w)), rng.standard_normal((nb, w))


class _as_is:
    def __enter__(self):
        pass

    def __exit__(self, *a):
        pass


def variant(lib, composed):
    """the call under test alone runs the composed form; its reference always comes from block_coldot / block_axpy_cols as
    the library runs them by default"""
    return U.block_fused_off(lib) if composed else _as_is()


class Basis:
    """nb slabs on the device, each `shift` doubles into its buffer, and their pointer table on the device"""

    def __init__(self, lib, V, shift):
        self.shift, self.V = shift, V
        self.bufs = [U.shifted(lib, v, shift) for v in V]
        self.table = Buf(lib, np.array([p for _, p in self.bufs], dtype=np.uint64))

    def ptr(self, i):
        return self.bufs[i][1]

    def unchanged(self):
        ok = all(same_bits(U.fetch(b, self.shift, v.shape), v) for (b, _), v in zip(self.bufs, self.V))
        return ok and same_bits(self.table.get(), np.array([p for _, p in self.bufs], dtype=np.uint64))

    def free(self):
        for b, _ in self.bufs:
            b.free()
        self.table.free()


def check_gs_dots(lib, w, n, nb, composed=False):
    """every row of H has the bits of block_coldot(V_i, W); two calls, and the two alignments, give one result"""
    V, W, _ = _slabs(n, w, nb, 90 + w)
    res = []
    for shift in (0, 1):
        bas = Basis(lib, V, shift)
        bw, pw = U.shifted(lib, W, shift)
        work = Buf(lib, np.full(nwg(n) * nb * w, SENTF))
        for rep in range(2):
            bh, ph = U.shifted(lib, np.full((nb, w), SENTF), shift)
            with variant(lib, composed):
                assert U.call(lib, "block_gs_dots", I=[nb, n, w], P=[bas.table, pw, ph, work]) == 1
            res.append(U.fetch(bh, shift, (nb, w)))
            bh.free()
        work.get()                                                       # its canaries
        bo, po = U.shifted(lib, np.full(w, SENTF), shift)
        for i in range(nb):
            assert U.call(lib, "block_coldot", I=[n, w], P=[bas.ptr(i), pw, po]) == 1
            ref = U.fetch(bo, shift, (w,))
            assert same_bits(res[-1][i], ref), "block_gs_dots row %d of %d, n %d, w %d, shift %d: not the bits of block_coldot" % (
                i, nb, n, w, shift)
        assert bas.unchanged() and same_bits(U.fetch(bw, shift, (n, w)), W), "block_gs_dots changed an input"
        for b_ in (bw, work, bo):
            b_.free()
        bas.free()
    assert same_bits(res[0], res[1]) and same_bits(res[2], res[3]), "block_gs_dots: two calls, two results"
    assert same_bits(res[0], res[2]), "block_gs_dots: the 16-byte path and the scalar path disagree"
    ref = np.stack([(v * W).sum(axis=0) for v in V])
    assert np.allclose(res[0], ref, rtol=0, atol=1e-9 * max(1.0, np.sqrt(n)) * 8)


def check_gs_update(lib, w, n, nb, norms, composed=False):
    """Y' has the bits of nb successive block_axpy_cols, norm2 those of block_coldot(Y', Y'); a column whose coefficients
    are all 0 keeps its bits; one coefficient is of denormal scale"""
    V, Y, Cf = _slabs(n, w, nb, 190 + w)
    Cf = Cf.copy()
    Cf[:, 3] = 0.0
    Cf[0, 5] = 1e-310
    for shift in (0, 1):
        bas = Basis(lib, V, shift)
        by, py = U.shifted(lib, Y, shift)
        bc, pcf = U.shifted(lib, Cf, shift)
        bn, pn = U.shifted(lib, np.full(w, SENTF), shift)
        work = Buf(lib, np.full(COLDOT_WG * w, SENTF))
        with variant(lib, composed):
            assert U.call(lib, "block_gs_update", I=[nb, n, w], P=[py, bas.table, pcf, pn if norms else None, work if norms else None]) == 1
        got = U.fetch(by, shift, (n, w))
        got_n = U.fetch(bn, shift, (w,))
        work.get()
        br, pr = U.shifted(lib, Y, shift)                                # the reference: one block_axpy_cols per slab
        for i in range(nb):
            assert U.call(lib, "block_axpy_cols", I=[n, w], P=[pr, bas.ptr(i), pcf + 8 * i * w]) == 1
        ref = U.fetch(br, shift, (n, w))
        what = "nb %d, n %d, w %d, shift %d, norms %s" % (nb, n, w, shift, norms)
        assert same_bits(got, ref), "block_gs_update: not the bits of successive block_axpy_cols: " + what
        assert same_bits(got[:, 3], Y[:, 3]), "block_gs_update changed a column whose coefficients are 0: " + what
        if norms:
            bo, po = U.shifted(lib, np.full(w, SENTF), shift)
            assert U.call(lib, "block_coldot", I=[n, w], P=[pr, pr, po]) == 1
            assert same_bits(got_n, U.fetch(bo, shift, (w,))), "block_gs_update: norm2 is not block_coldot(Y', Y'): " + what
            bo.free()
        else:
            assert same_bits(got_n, np.full(w, SENTF)), "block_gs_update wrote norm2 without being asked: " + what
        assert bas.unchanged() and same_bits(U.fetch(bc, shift, (nb, w)), Cf), "block_gs_update changed an input"
        for b_ in (by, bc, bn, work, br):
            b_.free()
        bas.free()


def check_scale_cols(lib, w, composed=False):
    rng = np.random.default_rng(290 + w)
    n = U.N_K
    X, c = rng.standard_normal((n, w)), rng.standard_normal(w)
    c[3] = 0.0
    ref = c[None, :] * X
    for shift in (0, 1):
        bx, px = U.shifted(lib, X, shift)
        bc, pcf = U.shifted(lib, c, shift)
        bo, po = U.shifted(lib, np.full((n, w), SENTF), shift)
        with variant(lib, composed):
            assert U.call(lib, "block_scale_cols", I=[n, w], P=[po, px, pcf]) == 1       # out of place
        got = U.fetch(bo, shift, (n, w))
        assert same_bits(got, ref), "block_scale_cols out of place, w %d, shift %d" % (w, shift)
        assert np.all(got[:, 3] == 0.0), "a zero coefficient did not give zeros"
        assert same_bits(U.fetch(bx, shift, (n, w)), X) and same_bits(U.fetch(bc, shift, (w,)), c)
        with variant(lib, composed):
            assert U.call(lib, "block_scale_cols", I=[n, w], P=[px, px, pcf]) == 1       # in place
        got = U.fetch(bx, shift, (n, w))
        assert same_bits(got, ref), "block_scale_cols in place, w %d, shift %d" % (w, shift)
        assert np.all(got[:, 3] == 0.0)
        for b_ in (bx, bc, bo):
            b_.free()


# ---------------------------------------------------------------------------------------------- the solve
@functools.lru_cache(maxsize=None)
def solve_columns(n, seeds):
    """m = 5: two seeded random columns, a multiple of the image A x_1 of column 1's solution, a zero column, a copy of
    column 1"""
    import scipy.sparse.linalg as sla
    mesh, dec, a, b = U.grid(n)
    N = mesh.nbNode
    c0, c1 = (np.random.default_rng(s).standard_normal(N) for s in seeds)
    x1 = sla.spsolve(a.tocsc(), c1)
    B = np.stack([c0, c1, 2.5 * (a @ x1), np.zeros(N), c1.copy()], axis=1)
    B.setflags(write=False)
    return B


_singles = {}


def singles_for(lib, n, argv, B):
    """KSPSolve_GenEO (-ksp_type gmres) on every column alone, on the PC of the block solve: (x, its, reason, history).
    Computed once per (library, case, options) and shared."""
    key = (id(lib), n, tuple(argv))
    if key not in _singles:
        pc = U.get_pc(lib, n, argv)
        N = B.shape[0]
        out = []
        for j in range(B.shape[1]):
            if j == 4:                                  # a copy of column 1: the same deterministic solve
                out.append(out[1])
                continue
            x, its, rnorm, reason = pc.solve(B[:, j], x0=np.zeros(N))
            out.append((x, its, reason, pc.residual_history().copy(), rnorm))
        _singles[key] = out
    return _singles[key]


def check_inputs(singles, rtol=1e-10):
    """on the single-vector histories alone: no column may hover at its threshold"""
    for j, (x, its, reason, hist, rnorm) in enumerate(singles):
        if its == 0:
            continue
        assert reason.startswith("KSP_CONVERGED"), (j, reason)
        thr = rtol * hist[0]
        assert hist[-1] < 0.95 * thr and hist[-2] > 1.05 * thr, \
            "bad input: column %d hovers at its threshold (%.3e, %.3e against %.3e): pick another seed" % (j, hist[-2], hist[-1], thr)


def measure_parity(lib, lvl, n, w, seeds, extra=()):
    """The block solve against the single-vector solve of every column; returns the largest per-column relative difference
    of the solutions after checking counts, reasons, the zero column and the copy."""
    argv = argv_for(lvl, w, extra)
    pc = U.get_pc(lib, n, argv)
    B = solve_columns(n, tuple(seeds))
    singles = singles_for(lib, n, argv, B)
    check_inputs(singles)
    X, its, rnorm, reasons = pc.mat_solve(B)
    print("KSPMatSolve gmres %s %d^3 w %d %s: its %s (single-vector %s)" % (lvl, n, w, list(extra), list(its), [s[1] for s in singles]))
    for j, (x, sits, sreason, hist, srn) in enumerate(singles):
        assert its[j] == sits and reasons[j] == sreason, (j, its[j], sits, reasons[j], sreason)
        if sits:
            # below the column's threshold, as the reason says.  (Not compared with the single-vector value: classical
            # Gram-Schmidt loses orthogonality like eps x the squared condition of the basis, which over a 30-step cycle
            # turns a rounding-level difference between the two paths into per cent of a residual 1e-10 below the start.)
            assert rnorm[j] <= 1e-10 * hist[0], (j, rnorm[j], hist[0])
    assert its[3] == 0 and reasons[3].startswith("KSP_CONVERGED") and not np.any(X[:, 3])
    assert same_bits(X[:, 4], X[:, 1]) and its[4] == its[1] and rnorm[4] == rnorm[1], "column 4 is a copy of column 1"
    a = U.grid(n)[2]
    for j in (0, 1, 2):
        assert np.linalg.norm(B[:, j] - a @ X[:, j]) <= 1e-7 * np.linalg.norm(B[:, j])
    return U.relcols(X, np.stack([s[0] for s in singles], axis=1))


def check_parity(lib, lvl, n, w, seeds, extra=()):
    err = measure_parity(lib, lvl, n, w, seeds, extra)
    print("block GMRES against KSPSolve, %s %d^3 w %d %s: %.3e (bound %.1e)" % (lvl, n, w, list(extra), err, PARITY_BOUND))
    assert err <= PARITY_BOUND
    return err


def check_restart_spread(lib, lvl, n, w, seeds):
    """with -ksp_gmres_restart 5 the columns stop in different cycles and in the middle of a cycle"""
    singles = singles_for(lib, n, argv_for(lvl, w, RESTART5), solve_columns(n, tuple(seeds)))
    its = [s[1] for s in singles if s[1] > 0]
    assert len({(i - 1) // 5 for i in its}) >= 2, "bad input: every column stops in the same cycle: %s" % its
    assert any(i % 5 for i in its), "bad input: no column stops in the middle of a cycle: %s" % its


def check_max_it(lib, lvl, n, w, seeds):
    pc = U.get_pc(lib, n, argv_for(lvl, w, ["-ksp_max_it", "3"]))
    B = solve_columns(n, tuple(seeds))
    X, its, rnorm, reasons = pc.mat_solve(B)
    for j in (0, 1, 2, 4):
        assert its[j] == 3 and reasons[j] == "KSP_DIVERGED_ITS", (j, its[j], reasons[j])
        x, sits, srn, sreason = pc.solve(B[:, j], x0=np.zeros(B.shape[0]))
        assert sits == 3 and sreason == reasons[j]
        assert np.linalg.norm(X[:, j] - x) <= PARITY_BOUND * np.linalg.norm(x)
    assert its[3] == 0 and reasons[3].startswith("KSP_CONVERGED") and not np.any(X[:, 3])


def check_fused_against_composed(lib, lvl, n, w, seeds, extra=(), restart=30):
    """GeneoSetKernelVariant("block_fused", 0): the same bits, and the Gram-Schmidt passes move to the composed counter"""
    pc = U.get_pc(lib, n, argv_for(lvl, w, extra))
    B = solve_columns(n, tuple(seeds))
    k0 = pc.block_krylov_info()
    X, its, rnorm, reasons = pc.mat_solve(B)
    k1 = pc.block_krylov_info()
    with U.block_fused_off(lib):
        X2, its2, rnorm2, reasons2 = pc.mat_solve(B)
    k2 = pc.block_krylov_info()
    assert list(its) == list(its2) and list(reasons) == list(reasons2)
    assert same_bits(rnorm, rnorm2), "rnorm differs between the fused and the composed form"
    assert same_bits(X, X2), "X differs between the fused and the composed form: %.3e" % U.relcols(X, X2)
    steps, cycles = int(max(its)), -(-int(max(its)) // restart)
    assert k1["gs_fused"] - k0["gs_fused"] == 2 * steps + cycles and k1["gs_composed"] == k0["gs_composed"], (k0, k1, steps, cycles)
    assert k2["gs_composed"] - k1["gs_composed"] == 2 * steps + cycles and k2["gs_fused"] == k1["gs_fused"], (k1, k2)
    assert k2["basis_slabs"] == min(restart, steps) + 1, (k2, steps)
    entries = B.shape[0] * w
    assert k2["basis_bytes"] >= 8.0 * k2["basis_slabs"] * entries
    return k2


def check_options(lib, n=12, w=16):
    """the new key, what it refuses, which method runs under which pair of keys -- and that a PC which has run block PCG
    alone holds no basis"""
    from geneo4petsc_amd.pc import GenEOError, GenEOPC
    p0 = GenEOPC(lib)
    assert "ksp_matsolve_type" not in p0.lib.PCGenEOGetOptionsString(p0.h).decode(), "the key shows although it is not set"
    assert "-ksp_matsolve_type" in p0.usage()
    for bad in ("foo", "", "GMRES", "fgmres"):
        with np.testing.assert_raises(GenEOError):
            p0.set_option("-ksp_matsolve_type", bad)
    with np.testing.assert_raises(GenEOError):
        p0.set_from_options(["-ksp_matsolve_type", "foo"])
    assert "ksp_matsolve_type" not in p0.options()
    p0.set_option("-ksp_matsolve_type", "gmres")
    assert p0.options()["ksp_matsolve_type"] == "gmres" and p0.options()["ksp_type"] == "gmres"
    p0.destroy()
    mesh, dec, a, b = U.grid(n)
    B = np.asarray(solve_columns(n, CASES[0][3])[:, :2])
    zeros = np.zeros(mesh.nbNode)
    loose = ["-ksp_rtol", "1e-3"]                      # which method runs is the point here, not how far it goes
    pc = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", w, U.SOLVE + loose), b)      # -ksp_type cg, the new key unset
    Xcg, its_cg, rn_cg, rs_cg = pc.mat_solve(B)
    x_cg, sits_cg, _, _ = pc.solve(B[:, 0], x0=zeros)
    assert sits_cg == its_cg[0]
    pc.set_option("-ksp_type", "gmres")                                           # on its own: refused, naming -ksp_type
    try:
        pc.mat_solve(B)
        raise AssertionError("KSPMatSolve_GenEO accepted -ksp_type gmres without -ksp_matsolve_type")
    except GenEOError as e:
        assert "-ksp_type" in str(e), str(e)
    pc.set_option("-ksp_matsolve_type", "cg")          # the block solve runs PCG, the single-vector solve GMRES
    X2, its2, rn2, rs2 = pc.mat_solve(B)
    assert same_bits(X2, Xcg) and list(its2) == list(its_cg) and same_bits(rn2, rn_cg) and list(rs2) == list(rs_cg)
    assert pc.block_krylov_info() == dict(basis_slabs=0, basis_bytes=0.0, gs_fused=0, gs_composed=0)
    x_gm, sits_gm, _, reason = pc.solve(B[:, 0], x0=zeros)
    hist = pc.residual_history()
    assert reason.startswith("KSP_CONVERGED") and np.all(np.diff(hist) <= 0.0), "not a GMRES history"
    assert not same_bits(x_gm, x_cg), "the single-vector solve did not change with -ksp_type"
    pc.set_option("-ksp_matsolve_type", "gmres")       # ... and now block GMRES, whatever -ksp_type says
    for ksp in ("cg", "gmres"):
        pc.set_option("-ksp_type", ksp)
        X3, its3, rn3, rs3 = pc.mat_solve(B)
        assert np.linalg.norm(X3[:, 0] - x_gm) <= 1e-9 * np.linalg.norm(x_gm), "the block solve is not GMRES under -ksp_type " + ksp
        info = pc.block_krylov_info()
        assert info["basis_slabs"] == int(max(its3)) + 1 and info["basis_bytes"] > 0.0, (info, list(its3))
    pc.set_option("-ksp_initial_guess_nonzero", "1")
    try:
        pc.mat_solve(B)
        raise AssertionError("block GMRES accepted -ksp_initial_guess_nonzero 1")
    except GenEOError as e:
        assert "-ksp_initial_guess_nonzero" in str(e), str(e)
    pc.destroy()
