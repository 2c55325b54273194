"""Shared checks of the right-preconditioned and the flexible GMRES of KSPSolve_GenEO (-ksp_pc_side right, -ksp_type fgmres)
and of their Gram-Schmidt primitives (csrc/krylov_dev.h), run by tests/test_krylov_right_host.py on the host twin and by
tests/test_gpu_krylov_right.py on the HIP library.  Every check takes the bound library; nothing here falls back from one to
the other.

Argument table of GeneoTestKrylovPrimitive (I = iarg, P = parg: device pointers):
  vec_gs_dots    I(nb, n)  P(V table, W, H, work)                       H: nb doubles; work: vec_dot_nwg(n) x nb doubles
  vec_gs_update  I(nb, n)  P(Y, V table, C, norm2 | NULL, work | NULL)  C: nb doubles; norm2: 1; work: vec_dot_nwg(n)
  vec_gs_group   -                                                      returns the group size G of vec_gs_dots
  vec_dot_nwg    I(n)                                                   returns the partial sums per vector of a pass
The V table is an array of nb vector pointers ON THE DEVICE.  GeneoSetKernelVariant("krylov_fused", 0) runs the composed
forms of core.cpp (one bk::dot / bk::axpy per vector), which a backend without the kernels (the host twin) always runs.

Bounds of the primitives (derived, not measured):
  vec_gs_dots    |H_i - exact| <= n 2^-53 sum_r |v_r w_r| x 1.01: the forward error bound of a sum of n rounded products in
                 any order (n - 1 additions and one product rounding per term, (1 + u)^n - 1 <= 1.01 n u for n u < 0.01),
                 the factor also covering the rounding of the numpy.longdouble reference.
  vec_gs_update  fused: every element is numpy's y = y + c_i * v_i, i in order, to the bit (two roundings per term).
                 composed: |Y' - exact| <= 2 nb 2^-53 (|Y| + sum_i |C_i V_i|) x 1.01 per element (at most two roundings per
                 term, each relative to a partial sum bounded by |Y| + sum |C_i V_i|; bk::axpy may contract to one).

Bounds of the solve against the numpy reference of this file (PARITY_BOUND).  The reference is a flexible GMRES with
right preconditioning that calls the library for PCApply_GenEO and MatMult_GenEO only, under -dls1_ksp_type chebyshev (a
fixed linear operator); it takes its residual norms from a least-squares solve of the Hessenberg system, not from Givens
rotations.  Library and reference run the same Krylov process and differ by rounding alone: the summation order of the dot
products and the way the small system is solved.  The inputs are checked first so that neither hovers at its threshold; the
iteration counts are then equal, and compared are
  hist   max_k |hist[k] - ref[k]| / ref[0]
  x      |x - x_ref| / |x_ref|
  rnorm  | rnorm - |b - A x|_2 | / |b|_2, A the assembled matrix in numpy
over CASES x (default restart, -ksp_gmres_restart 5) x (-ksp_initial_guess_nonzero 0, 1) x (fgmres, gmres + right).  The
largest of each was measured on the host twin and on an MI355X (profiles/r10_right_gmres.md); the bound is 100 x the larger
of the two, and never looser than 1e-7."""
import ctypes as C
import functools

import numpy as np

import block_rhs_util as U
from primitive_cases import SENTF, Buf, same_bits

LD = np.longdouble
#                       hist      x         rnorm
MEASURED_HOST = dict(hist=1.4e-10, x=3.0e-13, rnorm=2.3e-16)     # host twin: 1.399e-10, 2.970e-13, 2.264e-16 (profiles/r10_right_gmres.md)
MEASURED_GPU = dict(hist=6.0e-11, x=1.8e-13, rnorm=6.3e-17)      # MI355X: 5.980e-11, 1.771e-13, 6.257e-17
PARITY_BOUND = {k: min(1e-7, 100.0 * max(MEASURED_HOST[k], MEASURED_GPU[k])) for k in MEASURED_HOST}

RTOL = 1e-8
BASE = ["-geneo_tau", "0.2", "-geneo_cut", "4", "-ksp_rtol", "%g" % RTOL, "-dls1_ksp_rtol", "1e-7"]
CHEB = ["-dls1_ksp_type", "chebyshev"]
# (level, grid) and per (restart, guess) the seed of the right-hand side (and of the guess) with the -ksp_rtol of the solve:
# picked on the host twin, on the reference alone, so that the stopping iteration is below the threshold and the one before
# it above it by the factor MARGIN or more, and so that with -ksp_gmres_restart 5 the solve needs more than one cycle and
# ends in the middle of one.  MARGIN is 2 where a step of the solve reduces the residual fourfold.  SRAS,1 and SORAS,H1
# never do on these grids (their steps reduce it 1.2 to 2.5 times, whatever the seed: profiles/r10_right_gmres.md), so no
# threshold can lie a factor 2 from both of its neighbours; there the margin is 1.25, seven orders of magnitude above the
# rounding differences the counts have to be safe from.
CASES = (("RAS,1", 12), ("RAS,1", 20), ("ORAS,1", 12), ("SRAS,1", 12), ("SORAS,H1", 12))
CONFIGS = ((30, 0), (30, 1), (5, 0), (5, 1))          # (restart, -ksp_initial_guess_nonzero)
MARGIN = {"SRAS,1": 1.25, "SORAS,H1": 1.25}           # every other level: 2
SEEDS = {
    ('RAS,1', 12, 30, 0): (1, 8.671e-09),
    ('RAS,1', 12, 30, 1): (1, 1.241e-07),
    ('RAS,1', 12, 5, 0): (2, 3.046e-08),
    ('RAS,1', 12, 5, 1): (5, 6.849e-08),
    ('RAS,1', 20, 30, 0): (1, 1.61e-07),
    ('RAS,1', 20, 30, 1): (1, 2.85e-07),
    ('RAS,1', 20, 5, 0): (27, 8.687e-09),
    ('RAS,1', 20, 5, 1): (27, 1.03e-08),
    ('ORAS,1', 12, 30, 0): (1, 8.671e-09),
    ('ORAS,1', 12, 30, 1): (1, 1.241e-07),
    ('ORAS,1', 12, 5, 0): (2, 3.046e-08),
    ('ORAS,1', 12, 5, 1): (5, 6.849e-08),
    ('SRAS,1', 12, 30, 0): (1, 4.508e-07),
    ('SRAS,1', 12, 30, 1): (1, 1.347e-09),
    ('SRAS,1', 12, 5, 0): (1, 1.348e-07),
    ('SRAS,1', 12, 5, 1): (1, 8.222e-08),
    ('SORAS,H1', 12, 30, 0): (1, 4.18e-07),
    ('SORAS,H1', 12, 30, 1): (1, 3.12e-07),
    ('SORAS,H1', 12, 5, 0): (1, 5.565e-07),
    ('SORAS,H1', 12, 5, 1): (1, 3.488e-08),
}
BIG = 1024 * 512 + 513                                # the first size tested past VEC_DOT_WG = 1024 ranges of 512 rows: longer ranges
NONLINEAR = (("RAS,1", 12), ("SRAS,1", 12))           # -dls1_ksp_type cg -dls1_ksp_rtol 1e-2 under fgmres


def call(lib, name, I=(), P=()):
    ia = (C.c_int * max(1, len(I)))(*[int(v) for v in I])
    da = (C.c_double * 1)(0.0)
    pa = (C.c_void_p * max(1, len(P)))(*[(p if (p is None or isinstance(p, int)) else p.ptr) for p in P])
    rc = lib.GeneoTestKrylovPrimitive(name.encode(), ia, da, pa)
    assert rc >= 0, "%s: rc %d (%s)" % (name, rc, lib.PCGenEOGetError(None).decode())
    return rc


def gs_group(lib):
    return call(lib, "vec_gs_group")


def nwg(lib, n):
    return call(lib, "vec_dot_nwg", I=[n])


class krylov_fused_off:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.GeneoSetKernelVariant(b"krylov_fused", 0) == 0

    def __exit__(self, *a):
        assert self.lib.GeneoSetKernelVariant(b"krylov_fused", 1) == 0


class _as_is:
    def __enter__(self):
        pass

    def __exit__(self, *a):
        pass


def variant(lib, composed):
    return krylov_fused_off(lib) if composed else _as_is()


def sizes(lib):
    """n: one row, around a wave, around the rows of a few workgroups, and the first size past VEC_DOT_WG ranges of the
    smallest length, where the ranges grow"""
    big = BIG
    assert nwg(lib, big) < -(-big // 512) and nwg(lib, big - 513) == (big - 513) // 512, "the ranges do not change where the test expects it"
    return (1, 63, 64, 65, 1023, 1025, big)


def widths(lib):
    g = gs_group(lib)
    return tuple(sorted({1, max(1, g - 1), g, g + 1, 2 * g + 1, 31}))


# ---------------------------------------------------------------------------------------------- the primitives alone
@functools.lru_cache(maxsize=2)
def _vectors(n, nb, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((nb, n))
    W = rng.standard_normal(n)
    c = rng.standard_normal(nb)
    for a in (V, W, c):
        a.setflags(write=False)
    return V, W, c


class Vectors:
    """the rows of V on the device, each `shift` doubles into its buffer; tables of their pointers in any order"""

    def __init__(self, lib, V, shift):
        self.lib, self.V, self.shift = lib, V, shift
        self.bufs = [U.shifted(lib, v, shift) for v in V]
        self.tables = []

    def table(self, order=None):
        order = range(len(self.bufs)) if order is None else order
        t = Buf(self.lib, np.array([self.bufs[i][1] for i in order], dtype=np.uint64))
        self.tables.append((t, t.get().copy()))
        return t

    def unchanged(self):
        return all(same_bits(U.fetch(b, self.shift, v.shape), v) for (b, _), v in zip(self.bufs, self.V)) and \
            all(same_bits(t.get(), h) for t, h in self.tables)

    def free(self):
        for b, _ in self.bufs:
            b.free()
        for t, _ in self.tables:
            t.free()


def dots_bound(V, W):
    n = V.shape[1]
    return n * 2.0 ** -53 * (np.abs(V).astype(LD) * np.abs(W).astype(LD)).sum(axis=1) * 1.01


def check_vec_dots(lib, n, composed=False):
    """vec_gs_dots at every width of widths(): against the longdouble dot products within the derived bound; and to the bit
    -- two calls, the two alignments, a row whatever the number of vectors (1 .. 31), a vector at every position of its
    group.  Inputs unchanged, nothing written outside H and work."""
    nbs, g = widths(lib), gs_group(lib)
    nbmax = max(nbs)
    V, W, _ = _vectors(n, nbmax, 1000 + n)
    exact = (V.astype(LD) * W.astype(LD)).sum(axis=1)
    bound = dots_bound(V, W)
    per_shift = []
    for shift in (0, 1):
        vec = Vectors(lib, V, shift)
        tab = vec.table()
        bw, pw = U.shifted(lib, W, shift)

        def run(table, nb):
            work = Buf(lib, np.full(nwg(lib, n) * nb, SENTF))
            bh, ph = U.shifted(lib, np.full(nb, SENTF), shift)
            with variant(lib, composed):
                assert call(lib, "vec_gs_dots", I=[nb, n], P=[table, pw, ph, work]) == 1
            h = U.fetch(bh, shift, (nb,))
            work.get()                                                   # its canaries
            bh.free()
            work.free()
            return h

        full = run(tab, nbmax)
        err = np.abs(full.astype(LD) - exact)
        assert (err <= bound).all(), "vec_gs_dots n %d, shift %d: error %.3e beyond the bound %.3e" % (
            n, shift, float(err.max()), float(bound[np.argmax(err - bound)]))
        assert same_bits(run(tab, nbmax), full), "vec_gs_dots n %d: two calls, two results" % n
        for nb in nbs:                                                   # the first nb pointers of the same table
            assert same_bits(run(tab, nb), full[:nb]), "vec_gs_dots n %d: row bits depend on nb (%d against %d)" % (n, nb, nbmax)
        for pos in range(min(g, nbmax)):                                 # vector 0 at every position of the first group
            order = [(i - pos) % g for i in range(g)]
            assert same_bits(run(vec.table(order), g)[pos], full[0]), "vec_gs_dots n %d: bits depend on the position %d in the group" % (n, pos)
        assert vec.unchanged() and same_bits(U.fetch(bw, shift, (n,)), W), "vec_gs_dots changed an input"
        per_shift.append(full)
        bw.free()
        vec.free()
    assert same_bits(per_shift[0], per_shift[1]), "vec_gs_dots n %d: the 16-byte path and the scalar path disagree" % n


def check_vec_update(lib, n, composed=False):
    """vec_gs_update at every width: fused -- numpy's separately rounded sequence to the bit and norm2 with the bits of
    vec_gs_dots(&Y', 1, Y'); composed -- within the derived bound.  A null norm2 writes neither norm2 nor work."""
    nbs = widths(lib)
    nbmax = max(nbs)
    V, Y, c = _vectors(n, nbmax, 2000 + n)
    c = c.copy()
    if nbmax > 2:
        c[2] = 0.0
    # per width, computed once: numpy's separately rounded sequence (fused), or the exact sums and their bound (composed)
    refs, exacts, bounds = {}, {}, {}
    if composed:
        ex, ab = Y.astype(LD), np.abs(Y)
        for i in range(nbmax):
            ex = ex + LD(c[i]) * V[i].astype(LD)
            ab = ab + np.abs(c[i]) * np.abs(V[i])
            if i + 1 in nbs:
                exacts[i + 1], bounds[i + 1] = ex, 2 * (i + 1) * 2.0 ** -53 * ab * 1.01
    else:
        ref = Y.copy()
        for i in range(nbmax):
            ref = ref + c[i] * V[i]
            if i + 1 in nbs:
                refs[i + 1] = ref
    for shift in (0, 1):
        vec = Vectors(lib, V, shift)
        tab = vec.table()
        bc, pcf = U.shifted(lib, c, shift)
        for nb in nbs:
            for norms in (True, False):
                by, py = U.shifted(lib, Y, shift)
                bn, pn = U.shifted(lib, np.full(1, SENTF), shift)
                work = Buf(lib, np.full(nwg(lib, n), SENTF))
                with variant(lib, composed):
                    assert call(lib, "vec_gs_update", I=[nb, n], P=[py, tab, pcf, pn if norms else None, work]) == 1   # work is given either way, as the driver does
                got = U.fetch(by, shift, (n,))
                got_n = U.fetch(bn, shift, (1,))
                left = work.get()
                what = "nb %d, n %d, shift %d, norms %s" % (nb, n, shift, norms)
                if composed:
                    err = np.abs(got.astype(LD) - exacts[nb])
                    assert (err <= bounds[nb]).all(), "vec_gs_update (composed) beyond its bound: %s: %.3e" % (what, float((err - bounds[nb]).max()))
                else:
                    assert same_bits(got, refs[nb]), "vec_gs_update: not numpy's separately rounded sequence: " + what
                if norms:
                    # the bits of vec_gs_dots(&Y', 1, Y') under the same variant, on the buffer the update left
                    t1 = Buf(lib, np.array([py], dtype=np.uint64))
                    w1 = Buf(lib, np.full(nwg(lib, n), SENTF))
                    bo, po = U.shifted(lib, np.full(1, SENTF), shift)
                    with variant(lib, composed):
                        assert call(lib, "vec_gs_dots", I=[1, n], P=[t1, py, po, w1]) == 1
                    assert same_bits(got_n, U.fetch(bo, shift, (1,))), "vec_gs_update: norm2 is not vec_gs_dots(&Y', 1, Y'): " + what
                    ex2 = (got.astype(LD) ** 2).sum()
                    assert abs(LD(got_n[0]) - ex2) <= n * 2.0 ** -53 * ex2 * 1.01, "vec_gs_update: norm2 beyond the bound: " + what
                    for b_ in (t1, w1, bo):
                        b_.free()
                else:
                    assert same_bits(got_n, np.full(1, SENTF)), "vec_gs_update wrote norm2 without being asked: " + what
                    assert same_bits(left, np.full(nwg(lib, n), SENTF)), "vec_gs_update wrote work without being asked: " + what
                for b_ in (by, bn, work):
                    b_.free()
        assert vec.unchanged() and same_bits(U.fetch(bc, shift, (nbmax,)), c), "vec_gs_update changed an input"
        bc.free()
        vec.free()


# ---------------------------------------------------------------------------------------------- options
def check_options(lib, n=12):
    from geneo4petsc_amd.pc import GenEOError, GenEOPC
    import cases
    p = GenEOPC(lib)
    before = p.lib.PCGenEOGetOptionsString(p.h).decode()
    assert "ksp_pc_side" not in before and "ksp_pc_side" not in p.options(), "the key shows although it is not set"
    assert "fgmres" in p.usage() and "-ksp_pc_side" in p.usage()
    p.set_option("-ksp_type", "fgmres")                                  # "unsupported -ksp_type fgmres" without the feature
    assert p.options()["ksp_type"] == "fgmres" and "ksp_pc_side" not in p.options()
    p.set_option("-ksp_pc_side", "right")                                # fgmres is right: saying so is fine
    try:
        p.set_option("-ksp_pc_side", "left")
        raise AssertionError("-ksp_type fgmres accepted -ksp_pc_side left")
    except GenEOError as e:
        assert "-ksp_pc_side" in str(e) and "fgmres" in str(e), str(e)
    p.set_option("-ksp_type", "gmres")
    assert p.options()["ksp_type"] == "gmres" and p.options()["ksp_pc_side"] == "right"
    assert p.lib.PCGenEOGetOptionsString(p.h).decode().endswith(";ksp_pc_side=right")
    for bad in ("up", "", "RIGHT"):
        try:
            p.set_option("-ksp_pc_side", bad)
            raise AssertionError("-ksp_pc_side %r was accepted" % bad)
        except GenEOError as e:
            assert "-ksp_pc_side" in str(e), str(e)
    try:
        p.set_option("-ksp_type", "cg")
        raise AssertionError("-ksp_type cg accepted -ksp_pc_side right")
    except GenEOError as e:
        assert "-ksp_pc_side" in str(e) and "cg" in str(e), str(e)
    assert p.options()["ksp_type"] == "gmres", "a refused value was stored"
    p.destroy()
    for argv in (["-ksp_type", "cg", "-ksp_pc_side", "right"], ["-ksp_pc_side", "right", "-ksp_type", "cg"],
                 ["-ksp_type", "fgmres", "-ksp_pc_side", "left"], ["-ksp_pc_side", "left", "-ksp_type", "fgmres"],
                 ["-ksp_pc_side", "up"]):
        q = GenEOPC(lib)
        try:
            q.set_from_options(argv)
            raise AssertionError("accepted: %s" % argv)
        except GenEOError as e:
            assert "-ksp_pc_side" in str(e), str(e)
        q.destroy()
    q = GenEOPC(lib)
    q.set_from_options(["-ksp_type", "gmres", "-ksp_pc_side", "left"])
    assert q.options()["ksp_pc_side"] == "left"
    q.set_option("-ksp_matsolve_type", "gmres")                          # the other key keeps its own two values
    for bad in ("fgmres", "GMRES", "foo", ""):
        with np.testing.assert_raises(GenEOError):
            q.set_option("-ksp_matsolve_type", bad)
    q.destroy()
    # the block solve refuses the side and keeps its message for fgmres; the efficient hybrid is refused at the solve
    mesh, dec, a, b = U.grid(n)
    B = np.random.default_rng(5).standard_normal((mesh.nbNode, 2))
    pc = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", 16, ["-ksp_rtol", "1e-3"]), b)
    for key, val, words, back in (("-ksp_type", "fgmres", ("has no block form", "fgmres"), "cg"),):
        pc.set_option(key, val)
        try:
            pc.mat_solve(B)
            raise AssertionError("KSPMatSolve_GenEO accepted %s %s" % (key, val))
        except GenEOError as e:
            assert all(w in str(e) for w in words), str(e)
        finally:
            pc.set_option(key, back)
    pc.set_option("-ksp_type", "gmres")
    pc.set_option("-ksp_matsolve_type", "gmres")
    pc.set_option("-ksp_pc_side", "right")
    try:
        pc.mat_solve(B)
        raise AssertionError("KSPMatSolve_GenEO accepted -ksp_pc_side right")
    except GenEOError as e:
        assert "-ksp_pc_side" in str(e), str(e)
    pc.destroy()
    pe = cases.run_pc(lib, mesh, dec, ["-geneo_lvl", "ASM,E1"] + BASE + CHEB + ["-ksp_type", "fgmres"], b)   # the set-up passes
    for extra in ((), (("-ksp_type", "gmres"), ("-ksp_pc_side", "right"))):
        for k, v in extra:
            pe.set_option(k, v)
        try:
            pe.solve(b)
            raise AssertionError("the efficient hybrid ran a right-preconditioned method")
        except GenEOError as e:
            assert "-geneo_lvl" in str(e) and ("-ksp_pc_side" in str(e) and "fgmres" in str(e)), str(e)
    assert pe.krylov_info()["basis_vectors"] == 0
    pe.set_option("-ksp_pc_side", "left")
    x, its, rnorm, reason = pe.solve(b)                                  # left GMRES runs on it as before
    assert reason.startswith("KSP_CONVERGED")
    pe.destroy()


# ---------------------------------------------------------------------------------------------- the solve
def argv_for(lvl, extra=()):
    return ["-geneo_lvl", lvl] + BASE + list(extra)


def rhs(n, seed):
    """(b, x0): a seeded random right-hand side and a seeded random guess"""
    N = U.grid(n)[0].nbNode
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N), rng.standard_normal(N)


def reference_fgmres(pc, b, x0, restart, guess, rtol=RTOL, atol=1e-50, max_it=10000):
    """Right-preconditioned flexible GMRES in numpy: classical Gram-Schmidt, the residual norm of every step from a
    least-squares solve of the (k + 1) x k Hessenberg system.  The library gives M^-1 v (PCApply_GenEO) and A z
    (MatMult_GenEO) and nothing else.  Returns (x, its, hist, cycles that updated x)."""
    x = x0.copy() if guess else np.zeros_like(b)
    hist, its, cycles, first = [], 0, 0, True
    while True:
        r = b - pc.matmult(x) if (guess or not first) else b.copy()
        beta = float(np.linalg.norm(r))
        if first:
            ttol = max(rtol * (float(np.linalg.norm(b)) if guess else beta), atol)
            hist.append(beta)
            if beta <= ttol:
                return x, its, np.array(hist), cycles
            first = False
        V, Z = [r / beta], []
        H = np.zeros((restart + 1, restart))
        k, done, y = 0, False, None
        while k < restart and its < max_it and not done:
            z = pc.apply(V[k])
            w = pc.matmult(z)
            h = np.array([v @ w for v in V])
            w = w - np.stack(V, axis=1) @ h
            hn = float(np.linalg.norm(w))
            H[:k + 1, k], H[k + 1, k] = h, hn
            Z.append(z)
            V.append(w / hn)
            k += 1
            its += 1
            e1 = np.zeros(k + 1)
            e1[0] = beta
            y = np.linalg.lstsq(H[:k + 1, :k], e1, rcond=None)[0]
            hist.append(float(np.linalg.norm(e1 - H[:k + 1, :k] @ y)))
            done = hist[-1] <= ttol
        x = x + np.stack(Z, axis=1) @ y
        cycles += 1
        if done or its >= max_it:
            return x, its, np.array(hist), cycles


def input_ok(hist, its, restart, guess, b, rtol=RTOL, margin=2.0):
    """On the reference's history alone: it stops clear of its threshold on both sides, and with a short restart after more
    than one cycle and in the middle of one.  Returns None, or what is wrong."""
    thr = rtol * (float(np.linalg.norm(b)) if guess else hist[0])
    if its < 2 or not (hist[-1] <= thr / margin and hist[-2] >= margin * thr):
        return "hovers at its threshold (%.3e, %.3e against %.3e)" % (hist[-2], hist[-1], thr)
    if restart < 30 and not (its > restart and its % restart):
        return "%d iterations: not more than one cycle of %d ending in its middle" % (its, restart)
    return None


_refs = {}


def reference_for(lib, lvl, n, restart, guess):
    """the reference solve of a case, on the Chebyshev PC of the case: computed once per library and shared, unchanged"""
    key = (id(lib), lvl, n, restart, guess)
    if key not in _refs:
        pc = U.get_pc(lib, n, argv_for(lvl, CHEB))
        seed, rtol = SEEDS[(lvl, n, restart, guess)]
        b, x0 = rhs(n, seed)
        x, its, hist, cycles = reference_fgmres(pc, b, x0, restart, guess, rtol=rtol)
        bad = input_ok(hist, its, restart, guess, b, rtol, MARGIN.get(lvl, 2.0))
        assert bad is None, "bad input %s %d^3 restart %d guess %d: %s: pick another seed" % (lvl, n, restart, guess, bad)
        for a in (x, hist, b, x0):
            a.setflags(write=False)
        _refs[key] = dict(x=x, its=its, hist=hist, cycles=cycles, b=b, x0=x0, rtol=rtol)
    return _refs[key]


def set_method(pc, method, restart, guess):
    if method == "fgmres":
        pc.set_option("-ksp_pc_side", "right")
        pc.set_option("-ksp_type", "fgmres")
    elif method == "right":
        pc.set_option("-ksp_type", "gmres")
        pc.set_option("-ksp_pc_side", "right")
    else:                                                                # "gmres" | "cg", left
        if pc.options().get("ksp_pc_side") == "right":
            pc.set_option("-ksp_type", "gmres")
            pc.set_option("-ksp_pc_side", "left")
        pc.set_option("-ksp_type", method)
    pc.set_option("-ksp_gmres_restart", restart)
    pc.set_option("-ksp_initial_guess_nonzero", guess)


def run(pc, method, restart, guess, b, x0, rtol=RTOL):
    set_method(pc, method, restart, guess)
    pc.set_option("-ksp_rtol", repr(float(rtol)))
    x, its, rnorm, reason = pc.solve(b, x0=x0.copy() if guess else np.zeros_like(b))
    return dict(x=x, its=its, rnorm=rnorm, reason=reason, hist=pc.residual_history().copy(), info=pc.krylov_info())


def measure_case(lib, lvl, n, restart, guess, method):
    """one method against the reference: counts and reasons asserted, the three differences returned"""
    ref = reference_for(lib, lvl, n, restart, guess)
    pc = U.get_pc(lib, n, argv_for(lvl, CHEB))
    got = run(pc, method, restart, guess, ref["b"], ref["x0"], ref["rtol"])
    a = U.grid(n)[2]
    b = ref["b"]
    assert got["reason"] == "KSP_CONVERGED_RTOL", got["reason"]
    assert got["its"] == ref["its"], "%s %s %d^3 restart %d guess %d: %d iterations, the reference %d" % (
        method, lvl, n, restart, guess, got["its"], ref["its"])
    assert len(got["hist"]) == len(ref["hist"]) == got["its"] + 1
    d = dict(hist=float(np.max(np.abs(got["hist"] - ref["hist"])) / ref["hist"][0]),
             x=float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"])),
             rnorm=float(abs(got["rnorm"] - np.linalg.norm(b - a @ got["x"])) / np.linalg.norm(b)))
    assert got["rnorm"] == got["hist"][-1]
    # the applications of the preconditioner and the operator products the driver implements
    cyc = ref["cycles"]
    restarts = cyc - 1 + (1 if guess else 0)             # residuals b - A x computed: every cycle but a first one from zero
    assert got["info"]["pc_applies"] == got["its"] + (cyc if method == "right" else 0), (got["info"], got["its"], cyc)
    assert got["info"]["mat_mults"] == got["its"] + restarts, (got["info"], got["its"], restarts)
    print("%-6s %-8s %2d^3 restart %2d guess %d: its %3d  hist %.3e  x %.3e  rnorm %.3e" % (
        method, lvl, n, restart, guess, got["its"], d["hist"], d["x"], d["rnorm"]))
    return d, got


def check_case(lib, lvl, n, restart, guess):
    """fgmres and gmres + right against the reference, and against each other: equal counts, histories within the bound"""
    out = {}
    for method in ("fgmres", "right"):
        d, got = measure_case(lib, lvl, n, restart, guess, method)
        for k, v in d.items():
            assert v <= PARITY_BOUND[k], "%s %s %d^3 restart %d guess %d: %s %.3e beyond %.1e" % (
                method, lvl, n, restart, guess, k, v, PARITY_BOUND[k])
        out[method] = got
    f, r = out["fgmres"], out["right"]
    assert f["its"] == r["its"]
    dh = float(np.max(np.abs(f["hist"] - r["hist"])) / r["hist"][0])
    assert dh <= PARITY_BOUND["hist"], "fgmres against gmres + right: histories differ by %.3e" % dh
    return out


def check_krylov_info(lib, lvl="RAS,1", n=12, on_gpu=False):
    """what the methods hold and which form of the Gram-Schmidt passes ran -- on PCs of their own, so that nothing is shared"""
    import cases
    mesh, dec, a, _ = U.grid(n)
    restart, guess = 30, 0
    ref = reference_for(lib, lvl, n, restart, guess)
    b, x0 = ref["b"], ref["x0"]
    infos = {}
    for method in ("right", "fgmres"):
        pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
        zero = pc.krylov_info()
        assert zero == dict(basis_vectors=0, basis_bytes=0.0, gs_fused=0, gs_composed=0, pc_applies=0, mat_mults=0), zero
        left = run(pc, "gmres", restart, guess, b, x0, ref["rtol"])      # a left solve allocates nothing for the new methods
        assert left["info"]["basis_vectors"] == 0 and left["info"]["basis_bytes"] == 0.0, left["info"]
        assert left["info"]["gs_fused"] == 0 and left["info"]["gs_composed"] == 0
        got = run(pc, method, restart, guess, b, x0, ref["rtol"])
        its, cyc = got["its"], ref["cycles"]
        assert its == ref["its"] and its <= restart
        passes = 2 * its + cyc                                           # dots and update of every step, the update of x per cycle
        fused, composed = (passes, 0) if on_gpu else (0, passes)
        assert got["info"]["gs_fused"] == fused and got["info"]["gs_composed"] == composed, (got["info"], passes)
        if on_gpu:
            with krylov_fused_off(lib):
                again = run(pc, method, restart, guess, b, x0, ref["rtol"])
            assert again["its"] == its
            assert again["info"]["gs_fused"] == passes and again["info"]["gs_composed"] == passes, again["info"]
            assert np.linalg.norm(again["x"] - got["x"]) <= PARITY_BOUND["x"] * np.linalg.norm(got["x"])
        infos[method] = got["info"]
        assert got["info"]["basis_bytes"] >= 8.0 * got["info"]["basis_vectors"] * mesh.nbNode
        pc.destroy()
    # gmres + right: the basis v_0 .. v_its and two scratch vectors (w, z); fgmres: the same basis, z_0 .. z_its-1 and w
    assert infos["right"]["basis_vectors"] == its + 1 + 2, (infos, its)
    assert infos["fgmres"]["basis_vectors"] == 2 * (infos["right"]["basis_vectors"] - 2), (infos, its)


def check_nonlinear(lib, lvl, n, seed=7):
    """-dls1_ksp_type cg -dls1_ksp_rtol 1e-2: every application of the preconditioner is another operator.  fgmres converges,
    and since A Z = V H holds for any Z its estimate is the true residual up to rounding."""
    pc = U.get_pc(lib, n, argv_for(lvl, ["-dls1_ksp_type", "cg", "-dls1_ksp_rtol", "1e-2"]))
    a = U.grid(n)[2]
    b, x0 = rhs(n, seed)
    got = run(pc, "fgmres", 30, 0, b, x0)
    true = float(np.linalg.norm(b - a @ got["x"]))
    nb = float(np.linalg.norm(b))
    print("fgmres, -dls1_ksp_rtol 1e-2, %s %d^3: its %d, rnorm %.3e, |b - A x| %.3e, |b| %.3e" % (lvl, n, got["its"], got["rnorm"], true, nb))
    assert got["reason"].startswith("KSP_CONVERGED"), got["reason"]
    assert true <= max(RTOL * nb, 1e-50) + PARITY_BOUND["rnorm"] * nb, (true, RTOL * nb)
    return got


def check_disturbs_nothing(lib, lvl, n, seed=11):
    """left gmres and cg before and after a right solve on the same PC, and on a fresh PC: the same counts and bits"""
    import cases
    mesh, dec, a, _ = U.grid(n)
    b, x0 = rhs(n, seed)
    methods = ("gmres", "cg") if lvl.startswith("SRAS") else ("gmres",)   # cg: the symmetric mode only
    pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
    before = {m: run(pc, m, 30, 1, b, x0) for m in methods}
    for m in ("right", "fgmres"):
        assert run(pc, m, 30, 1, b, x0)["reason"].startswith("KSP_CONVERGED")
    assert pc.krylov_info()["basis_vectors"] > 0
    after = {m: run(pc, m, 30, 1, b, x0) for m in methods}
    pc.destroy()
    fresh_pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
    fresh = {m: run(fresh_pc, m, 30, 1, b, x0) for m in methods}
    fresh_pc.destroy()
    for m in methods:
        for other, what in ((after[m], "after a right solve"), (fresh[m], "on a fresh PC")):
            assert before[m]["its"] == other["its"] and before[m]["reason"] == other["reason"], (m, what)
            assert same_bits(before[m]["hist"], other["hist"]) and same_bits(before[m]["x"], other["x"]), \
                "left %s %s: not the same bits" % (m, what)
        assert before[m]["reason"].startswith("KSP_CONVERGED")
