"""Shared checks of the flexible CG of KSPSolve_GenEO (-ksp_type fcg) and of its step primitive (csrc/krylov_dev.h:
vec_fcg_step), run by tests/test_fcg_host.py on the host twin and by tests/test_gpu_fcg.py on the HIP library.  Every check
takes the bound library; nothing here falls back from one to the other.

Argument table of GeneoTestKrylovPrimitive (I = iarg, P = parg: device pointers), beside tests/krylov_right_util.py's:
  vec_fcg_step   I(n)  P(x, r, p, w, S, norm2 | NULL, work | NULL)      S: [eta, pi]; norm2: 1; work: vec_dot_nwg(n)
GeneoSetKernelVariant("krylov_fused", 0) runs the composed form of core.cpp (download S, bk::axpy, bk::axpy, bk::dot),
which a backend without the kernel (the host twin) always runs.

Bounds of the primitive (derived, not measured), alpha = S[1] / S[0] in numpy:
  fused     x' = x + alpha * p and r' = r - alpha * w are numpy's separately rounded expressions to the bit; norm2 has the
            bits of vec_gs_dots(&r', 1, r').
  composed  |x' - exact| <= 2 x 2^-53 (|x| + |alpha p|) x 1.01 per element, and the like for r (at most two roundings, each
            relative to a value bounded by |x| + |alpha p|; bk::axpy may contract to one); |norm2 - sum r'^2| <= n 2^-53
            sum r'^2 x 1.01 (krylov_right_util.py's bound of a sum of n rounded products).

Bounds of the solve against the numpy reference of this file (PARITY_BOUND).  The reference is a flexible CG that calls the
library for PCApply_GenEO and MatMult_GenEO only, under -dls1_ksp_type chebyshev (a fixed linear operator).  Library and
reference run the same process and differ by rounding alone (the summation order of the dot products).  The inputs are
checked first, on the reference's history alone, so that neither hovers at its threshold; the iteration counts are then
equal, and compared are
  hist   max_k |hist[k] - ref[k]| / ref[0]
  x      |x - x_ref| / |x_ref|
  rnorm  | rnorm - |b - A x|_2 | / |b|_2, A the assembled matrix in numpy (-ksp_norm_type unpreconditioned only)
over CASES x (-ksp_initial_guess_nonzero 0, 1) x (preconditioned, unpreconditioned), over the truncation cases (TRUNC) and,
for hist, over fcg against the library's own cg (EQUALS_CG).  The largest of each was measured on the host twin and on an
MI355X (profiles/r11_fcg.md); the bound is 100 x the larger of the two, and never looser than 1e-7."""
import functools

import numpy as np

import block_rhs_util as U
import krylov_right_util as K
from primitive_cases import SENTF, Buf, same_bits

LD = np.longdouble
#                       hist      x         rnorm
MEASURED_HOST = dict(hist=9.7e-10, x=4.3e-12, rnorm=9.0e-17)     # host twin: 9.692e-10, 4.277e-12, 8.981e-17 (profiles/r11_fcg.md)
MEASURED_GPU = dict(hist=2.1e-10, x=2.5e-13, rnorm=5.0e-17)      # MI355X: 2.070e-10, 2.410e-13, 4.943e-17
PARITY_BOUND = {k: min(1e-7, 100.0 * max(MEASURED_HOST[k], MEASURED_GPU[k])) for k in MEASURED_HOST}

BASE = ["-geneo_tau", "0.2", "-geneo_cut", "4", "-ksp_rtol", "1e-8", "-dls1_ksp_rtol", "1e-7"]
CHEB = ["-dls1_ksp_type", "chebyshev"]
CASES = (("ASM,1", 12), ("SRAS,1", 12), ("SORAS,H1", 12), ("ASM,1", 20))
CONFIGS = ((0, "preconditioned"), (1, "preconditioned"), (0, "unpreconditioned"), (1, "unpreconditioned"))
# (level, grid, guess, norm) -> the seed of the right-hand side (and of the guess) with the -ksp_rtol of the solve: picked on
# the host twin, on the reference alone (input_ok), so that the stopping iterate is below the threshold and every one before
# it above it by the margin -- 2 where the step into the stopping iterate reduces the norm fourfold, 1.25 otherwise.
SEEDS = {
    ('ASM,1', 12, 0, 'preconditioned'): (1, 9.322e-09),
    ('ASM,1', 12, 1, 'preconditioned'): (1, 1.216e-10),
    ('ASM,1', 12, 0, 'unpreconditioned'): (1, 1.14e-08),
    ('ASM,1', 12, 1, 'unpreconditioned'): (1, 1.35e-10),
    ('SRAS,1', 12, 0, 'preconditioned'): (1, 4.807e-09),
    ('SRAS,1', 12, 1, 'preconditioned'): (1, 9.825e-08),
    ('SRAS,1', 12, 0, 'unpreconditioned'): (1, 8.734e-10),
    ('SRAS,1', 12, 1, 'unpreconditioned'): (1, 1.043e-07),
    ('SORAS,H1', 12, 0, 'preconditioned'): (1, 2.617e-08),
    ('SORAS,H1', 12, 1, 'preconditioned'): (1, 2.434e-10),
    ('SORAS,H1', 12, 0, 'unpreconditioned'): (1, 1.324e-08),
    ('SORAS,H1', 12, 1, 'unpreconditioned'): (1, 4.183e-08),
    ('ASM,1', 20, 0, 'preconditioned'): (1, 9.423e-10),
    ('ASM,1', 20, 1, 'preconditioned'): (1, 1.431e-08),
    ('ASM,1', 20, 0, 'unpreconditioned'): (1, 8.279e-09),
    ('ASM,1', 20, 1, 'unpreconditioned'): (1, 1.359e-07),
}
TRUNC_LVL, TRUNC_N, TRUNC_ITS, TRUNC_SEED = "RAS,1", 12, 12, 1
TRUNC = tuple((m, t) for m in (1, 3, 30) for t in ("notay", "standard"))
EQUALS_CG = (("ASM,1", 12), ("SORAS,H1", 12))         # asserted; SRAS,1 is measured and printed only
NONLINEAR = (("SRAS,1", 12), ("ASM,1", 12))           # -dls1_ksp_type cg -dls1_ksp_rtol 1e-2 under fcg


def argv_for(lvl, extra=()):
    return ["-geneo_lvl", lvl] + BASE + list(extra)


# ---------------------------------------------------------------------------------------------- the window, in Python
def window(i, mmax, trunc):
    mi = max(1, i % (mmax + 1)) if trunc == "notay" else mmax
    return min(i, mi)


def max_window(its, mmax, trunc):
    return max([window(i, mmax, trunc) for i in range(its)] + [0])


# ---------------------------------------------------------------------------------------------- the step alone
@functools.lru_cache(maxsize=2)
def _step_vectors(n):
    rng = np.random.default_rng(3000 + n)
    v = [rng.standard_normal(n) for _ in range(4)]
    for a in v:
        a.setflags(write=False)
    return v


def check_fcg_step(lib, n, composed=False):
    """vec_fcg_step on x, r, p, w of n rows, the buffers 0 and 1 doubles into their allocations, with and without norm2;
    eta = 0, eta < 0 and eta = NaN change nothing; p, w and S are never written."""
    x, r, p, w = _step_vectors(n)
    nw = K.nwg(lib, n)
    S_good = np.array([1.7320508075688772, -0.8414709848078965])
    for S in (S_good, np.array([0.0, 1.0]), np.array([-2.0, 1.0]), np.array([np.nan, 1.0])):
        go = bool(S[0] > 0.0)
        with np.errstate(all="ignore"):
            alpha = S[1] / S[0]
        for shift in (0, 1):
            for norms in (True, False):
                bx, px = U.shifted(lib, x, shift)
                br, pr = U.shifted(lib, r, shift)
                bp, pp = U.shifted(lib, p, shift)
                bw, pw = U.shifted(lib, w, shift)
                bs, ps = U.shifted(lib, S, shift)
                bn, pn = U.shifted(lib, np.full(1, SENTF), shift)
                work = Buf(lib, np.full(nw, SENTF))
                with K.variant(lib, composed):
                    assert K.call(lib, "vec_fcg_step", I=[n], P=[px, pr, pp, pw, ps, pn if norms else None, work]) == 1
                gx, gr = U.fetch(bx, shift, (n,)), U.fetch(br, shift, (n,))
                gn, left = U.fetch(bn, shift, (1,)), work.get()
                what = "n %d, shift %d, norms %s, S %s" % (n, shift, norms, S)
                assert same_bits(U.fetch(bp, shift, (n,)), p) and same_bits(U.fetch(bw, shift, (n,)), w) and \
                    same_bits(U.fetch(bs, shift, (2,)), S), "vec_fcg_step changed an input: " + what
                if not go:
                    assert same_bits(gx, x) and same_bits(gr, r), "vec_fcg_step wrote x or r although eta is not positive: " + what
                elif composed:
                    ex, er = x.astype(LD) + LD(alpha) * p.astype(LD), r.astype(LD) - LD(alpha) * w.astype(LD)
                    bx_ = 2 * 2.0 ** -53 * (np.abs(x) + np.abs(alpha * p)) * 1.01
                    br_ = 2 * 2.0 ** -53 * (np.abs(r) + np.abs(alpha * w)) * 1.01
                    assert (np.abs(gx.astype(LD) - ex) <= bx_).all() and (np.abs(gr.astype(LD) - er) <= br_).all(), \
                        "vec_fcg_step (composed) beyond its bound: " + what
                else:
                    assert same_bits(gx, x + alpha * p), "vec_fcg_step: x is not numpy's x + alpha * p: " + what
                    assert same_bits(gr, r - alpha * w), "vec_fcg_step: r is not numpy's r - alpha * w: " + what
                if norms:
                    ex2 = (gr.astype(LD) ** 2).sum()
                    assert abs(LD(gn[0]) - ex2) <= n * 2.0 ** -53 * ex2 * 1.01, "vec_fcg_step: norm2 beyond the bound: " + what
                    if not composed:
                        # the bits of vec_gs_dots(&r', 1, r') on the buffer the step left
                        t1 = Buf(lib, np.array([pr], dtype=np.uint64))
                        w1 = Buf(lib, np.full(nw, SENTF))
                        bo, po = U.shifted(lib, np.full(1, SENTF), shift)
                        assert K.call(lib, "vec_gs_dots", I=[1, n], P=[t1, pr, po, w1]) == 1
                        assert same_bits(gn, U.fetch(bo, shift, (1,))), "vec_fcg_step: norm2 is not vec_gs_dots(&r', 1, r'): " + what
                        for b_ in (t1, w1, bo):
                            b_.free()
                else:
                    assert same_bits(gn, np.full(1, SENTF)), "vec_fcg_step wrote norm2 without being asked: " + what
                    assert same_bits(left, np.full(nw, SENTF)), "vec_fcg_step wrote work without being asked: " + what
                for b_ in (bx, br, bp, bw, bs, bn, work):
                    b_.free()


# ---------------------------------------------------------------------------------------------- options
def _refused(fn, *words):
    from geneo4petsc_amd.pc import GenEOError
    try:
        fn()
    except GenEOError as e:
        assert all(w in str(e) for w in words), str(e)
        return
    raise AssertionError("accepted, where a refusal naming %s was expected" % (words,))


def check_options(lib, n=12):
    from geneo4petsc_amd.pc import GenEOPC
    import cases
    new_keys = ("ksp_fcg_mmax", "ksp_fcg_truncation_type", "ksp_norm_type")
    p = GenEOPC(lib)
    before = p.lib.PCGenEOGetOptionsString(p.h).decode()
    assert not any(k in before for k in new_keys) and not any(k in p.options() for k in new_keys), "a key shows although it is not set"
    for word in ("fcg", "-ksp_fcg_mmax", "-ksp_fcg_truncation_type", "-ksp_norm_type"):
        assert word in p.usage(), word
    p.set_option("-ksp_type", "fcg")                                     # "unsupported -ksp_type fcg" without the feature
    assert p.options()["ksp_type"] == "fcg"
    assert p.lib.PCGenEOGetOptionsString(p.h).decode() == before.replace("ksp_type=gmres", "ksp_type=fcg"), "another key moved"
    _refused(lambda: p.set_option("-ksp_pc_side", "right"), "-ksp_pc_side", "fcg", "left-preconditioned")
    assert "ksp_pc_side" not in p.options(), "a refused value was stored"
    p.set_option("-ksp_pc_side", "left")                                 # fcg is left: saying so is fine
    for bad in ("0", "-1", "x", "", "2.5"):
        _refused(lambda: p.set_option("-ksp_fcg_mmax", bad), "-ksp_fcg_mmax")
    for bad in ("Notay", "", "none"):
        _refused(lambda: p.set_option("-ksp_fcg_truncation_type", bad), "-ksp_fcg_truncation_type")
    for bad in ("natural", "none", "", "UNPRECONDITIONED"):
        _refused(lambda: p.set_option("-ksp_norm_type", bad), "-ksp_norm_type")
    assert not any(k in p.options() for k in new_keys), "a refused value was stored"
    p.set_option("-ksp_fcg_mmax", 7)
    p.set_option("-ksp_fcg_truncation_type", "standard")
    p.set_option("-ksp_norm_type", "unpreconditioned")
    o = p.options()
    assert o["ksp_fcg_mmax"] == 7 and o["ksp_fcg_truncation_type"] == "standard" and o["ksp_norm_type"] == "unpreconditioned", o
    assert p.lib.PCGenEOGetOptionsString(p.h).decode().endswith(
        ";ksp_pc_side=left;ksp_fcg_mmax=7;ksp_fcg_truncation_type=standard;ksp_norm_type=unpreconditioned")
    p.set_option("-ksp_norm_type", "preconditioned")
    p.set_option("-ksp_fcg_truncation_type", "notay")
    p.destroy()
    p = GenEOPC(lib)
    p.set_option("-ksp_pc_side", "right")
    _refused(lambda: p.set_option("-ksp_type", "fcg"), "-ksp_pc_side", "fcg", "left-preconditioned")
    assert p.options()["ksp_type"] == "gmres", "a refused value was stored"
    p.destroy()
    for argv in (["-ksp_type", "fcg", "-ksp_pc_side", "right"], ["-ksp_pc_side", "right", "-ksp_type", "fcg"]):
        q = GenEOPC(lib)
        _refused(lambda: q.set_from_options(argv), "-ksp_pc_side", "fcg")
        q.destroy()
    for argv in (["-ksp_fcg_mmax", "0"], ["-ksp_fcg_truncation_type", "both"], ["-ksp_norm_type", "natural"]):
        q = GenEOPC(lib)
        _refused(lambda: q.set_from_options(argv), argv[0])
        q.destroy()
    # the block solve keeps its refusal; unpreconditioned with another method is refused at the solve, by both names
    mesh, dec, a, b = U.grid(n)
    B = np.random.default_rng(5).standard_normal((mesh.nbNode, 2))
    pc = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", 16, ["-ksp_rtol", "1e-3"]), b)
    pc.set_option("-ksp_type", "fcg")
    _refused(lambda: pc.mat_solve(B), "has no block form", "fcg")
    pc.set_option("-ksp_norm_type", "unpreconditioned")                  # accepted when set, whatever the method
    for method in ("cg", "gmres"):
        pc.set_option("-ksp_type", method)
        _refused(lambda: pc.solve(b), "-ksp_norm_type", "-ksp_type")
    pc.set_option("-ksp_type", "fcg")
    x, its, rnorm, reason = pc.solve(b, x0=np.zeros_like(b))
    assert reason.startswith("KSP_CONVERGED"), reason
    pc.set_option("-ksp_norm_type", "preconditioned")
    pc.set_option("-ksp_type", "cg")
    assert pc.solve(b, x0=np.zeros_like(b))[3].startswith("KSP_CONVERGED")
    pc.destroy()


# ---------------------------------------------------------------------------------------------- the solve
def rhs(n, seed):
    return K.rhs(n, seed)


def reference_fcg(pc, b, x0, guess, mmax=30, trunc="notay", norm="preconditioned", rtol=1e-8, atol=1e-50, dtol=1e5, max_it=10000):
    """Flexible CG in numpy, statement for statement what the issue's method does; the library gives M^-1 r (PCApply_GenEO)
    and A p (MatMult_GenEO) and nothing else.  Returns (x, its, hist, reason)."""
    x = x0.copy() if guess else np.zeros_like(b)
    r = b - pc.matmult(x) if guess else b.copy()
    P, W, eta = {}, {}, {}
    hist = []

    def test(it, rn, ref0):
        nonlocal ttol, rn0
        if it == 0:
            rn0 = ref0
            ttol = max(rtol * rn0, atol)
        if rn <= ttol:
            return "KSP_CONVERGED_RTOL"
        if rn >= dtol * rn0:
            return "KSP_DIVERGED_DTOL"
        return None
    ttol = rn0 = 0.0

    def step(i, z):
        nonlocal x, r
        m = window(i, mmax, trunc)
        p = z.copy()
        for k in range(i - m, i):
            p = p - ((W[k] @ z) / eta[k]) * P[k]
        w = pc.matmult(p)
        eta[i] = float(w @ p)
        alpha = float(r @ p) / eta[i]
        x = x + alpha * p
        r = r - alpha * w
        P[i], W[i] = p, w
        for k in [k for k in P if k < i + 1 - mmax]:
            del P[k], W[k]

    if norm == "unpreconditioned":
        rn = float(np.linalg.norm(r))
        hist.append(rn)
        reason = test(0, rn, float(np.linalg.norm(b)) if guess else rn)
        i = 0
        while reason is None and i < max_it:
            step(i, pc.apply(r))
            i += 1
            hist.append(float(np.linalg.norm(r)))
            reason = test(i, hist[-1], None)
        return x, i, np.array(hist), reason or "KSP_DIVERGED_ITS"
    i = 0
    while True:
        z = pc.apply(r)
        hist.append(float(np.linalg.norm(z)))
        reason = test(i, hist[-1], (float(np.linalg.norm(pc.apply(b))) if guess else hist[-1]) if i == 0 else None)
        if reason is None and i >= max_it:
            reason = "KSP_DIVERGED_ITS"
        if reason is not None:
            return x, i, np.array(hist), reason
        step(i, z)
        i += 1


def threshold(pc, b, guess, norm, hist0, rtol):
    if not guess:
        return rtol * hist0
    return rtol * float(np.linalg.norm(pc.apply(b)) if norm == "preconditioned" else np.linalg.norm(b))


def input_ok(hist, its, thr):
    """On a history alone: the stopping iterate lies below the threshold and every one before it above, by a margin of 2
    where the last step reduces the norm fourfold and 1.25 otherwise.  Returns None, or what is wrong."""
    if its < 2 or len(hist) != its + 1:
        return "%d iterations, %d norms" % (its, len(hist))
    margin = 2.0 if hist[-2] >= 4.0 * hist[-1] else 1.25
    if not (hist[-1] <= thr / margin and min(hist[:-1]) >= margin * thr):
        return "hovers at its threshold (%.3e, %.3e against %.3e, margin %.2f)" % (min(hist[:-1]), hist[-1], thr, margin)
    return None


_refs = {}


def reference_for(lib, lvl, n, guess, norm):
    """the reference solve of a case, on the Chebyshev PC of the case: computed once per library and shared, unchanged"""
    key = (id(lib), lvl, n, guess, norm)
    if key not in _refs:
        pc = U.get_pc(lib, n, argv_for(lvl, CHEB))
        seed, rtol = SEEDS[(lvl, n, guess, norm)]
        b, x0 = rhs(n, seed)
        x, its, hist, reason = reference_fcg(pc, b, x0, guess, norm=norm, rtol=rtol)
        bad = input_ok(hist, its, threshold(pc, b, guess, norm, hist[0], rtol))
        assert reason == "KSP_CONVERGED_RTOL" and bad is None, "bad input %s %d^3 guess %d %s: %s %s: pick another seed" % (
            lvl, n, guess, norm, reason, bad)
        for a in (x, hist, b, x0):
            a.setflags(write=False)
        _refs[key] = dict(x=x, its=its, hist=hist, reason=reason, b=b, x0=x0, rtol=rtol)
    return _refs[key]


def set_method(pc, method, guess, norm="preconditioned", mmax=30, trunc="notay"):
    if pc.options().get("ksp_pc_side") == "right":
        pc.set_option("-ksp_type", "gmres")
        pc.set_option("-ksp_pc_side", "left")
    if method != "fcg":
        norm = "preconditioned"
    pc.set_option("-ksp_type", method)
    pc.set_option("-ksp_norm_type", norm)
    pc.set_option("-ksp_fcg_mmax", mmax)
    pc.set_option("-ksp_fcg_truncation_type", trunc)
    pc.set_option("-ksp_initial_guess_nonzero", guess)


def run(pc, method, guess, b, x0, rtol, norm="preconditioned", mmax=30, trunc="notay", max_it=10000):
    set_method(pc, method, guess, norm, mmax, trunc)
    pc.set_option("-ksp_rtol", repr(float(rtol)))
    pc.set_option("-ksp_max_it", max_it)
    x, its, rnorm, reason = pc.solve(b, x0=x0.copy() if guess else np.zeros_like(b))
    return dict(x=x, its=its, rnorm=rnorm, reason=reason, hist=pc.residual_history().copy(), info=pc.krylov_info(),
                fcg=pc.fcg_info())


def differences(got, ref, a, b, norm):
    d = dict(hist=float(np.max(np.abs(got["hist"] - ref["hist"])) / ref["hist"][0]),
             x=float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"])))
    if norm == "unpreconditioned":
        d["rnorm"] = float(abs(got["rnorm"] - np.linalg.norm(b - a @ got["x"])) / np.linalg.norm(b))
    return d


def measure_case(lib, lvl, n, guess, norm):
    """fcg against the reference: counts, reasons and the counters the driver implies asserted, the differences returned"""
    ref = reference_for(lib, lvl, n, guess, norm)
    pc = U.get_pc(lib, n, argv_for(lvl, CHEB))
    got = run(pc, "fcg", guess, ref["b"], ref["x0"], ref["rtol"], norm)
    what = "fcg %s %d^3 guess %d %s" % (lvl, n, guess, norm)
    assert got["reason"] == ref["reason"] == "KSP_CONVERGED_RTOL", (what, got["reason"])
    assert got["its"] == ref["its"], "%s: %d iterations, the reference %d" % (what, got["its"], ref["its"])
    assert len(got["hist"]) == len(ref["hist"]) == got["its"] + 1 and got["rnorm"] == got["hist"][-1]
    d = differences(got, ref, U.grid(n)[2], ref["b"], norm)
    its = got["its"]
    # preconditioned: z of every iterate, the stopping one included, and M^-1 b with a guess; unpreconditioned: one per step
    assert got["info"]["pc_applies"] == (its + 1 + guess if norm == "preconditioned" else its), (what, got["info"], its)
    assert got["info"]["mat_mults"] == its + guess, (what, got["info"], its)
    assert got["fcg"]["max_window"] == max_window(its, 30, "notay"), (what, got["fcg"], its)
    print("%-8s %2d^3 guess %d %-16s: its %3d  " % (lvl, n, guess, norm, its) + "  ".join("%s %.3e" % kv for kv in d.items()))
    return d, got


def check_case(lib, lvl, n, guess, norm):
    d, got = measure_case(lib, lvl, n, guess, norm)
    for k, v in d.items():
        assert v <= PARITY_BOUND[k], "fcg %s %d^3 guess %d %s: %s %.3e beyond %.1e" % (lvl, n, guess, norm, k, v, PARITY_BOUND[k])
    return got


# ---------------------------------------------------------------------------------------------- truncation
_trunc_refs = {}


def trunc_reference(lib, mmax, trunc):
    key = (id(lib), mmax, trunc)
    if key not in _trunc_refs:
        pc = U.get_pc(lib, TRUNC_N, argv_for(TRUNC_LVL, CHEB))
        b, x0 = rhs(TRUNC_N, TRUNC_SEED)
        x, its, hist, reason = reference_fcg(pc, b, x0, 0, mmax=mmax, trunc=trunc, rtol=1e-30, max_it=TRUNC_ITS)
        for a in (x, hist, b):
            a.setflags(write=False)
        _trunc_refs[key] = dict(x=x, its=its, hist=hist, reason=reason, b=b, x0=x0)
    return _trunc_refs[key]


def measure_truncation(lib, mmax, trunc):
    """RAS,1: a fixed linear non-symmetric M^-1, where the window matters.  12 iterations of library and reference."""
    ref = trunc_reference(lib, mmax, trunc)
    assert ref["reason"] == "KSP_DIVERGED_ITS" and ref["its"] == TRUNC_ITS, \
        "the reference of mmax %d %s ended with %s after %d" % (mmax, trunc, ref["reason"], ref["its"])   # e.g. -ksp_divtol
    pc = U.get_pc(lib, TRUNC_N, argv_for(TRUNC_LVL, CHEB))
    got = run(pc, "fcg", 0, ref["b"], ref["x0"], 1e-30, mmax=mmax, trunc=trunc, max_it=TRUNC_ITS)
    assert got["reason"] == "KSP_DIVERGED_ITS" and got["its"] == TRUNC_ITS, (got["reason"], got["its"])
    assert len(got["hist"]) == len(ref["hist"]) == TRUNC_ITS + 1
    assert got["fcg"]["max_window"] == max_window(TRUNC_ITS, mmax, trunc), (got["fcg"], mmax, trunc)
    assert got["fcg"]["directions"] == min(TRUNC_ITS, mmax + 1), (got["fcg"], mmax)
    d = differences(got, ref, None, None, "preconditioned")
    print("truncation mmax %2d %-8s: hist %.3e  x %.3e  (last norm %.3e of %.3e)" % (
        mmax, trunc, d["hist"], d["x"], ref["hist"][-1], ref["hist"][0]))
    return d


def check_truncation(lib, mmax, trunc):
    d = measure_truncation(lib, mmax, trunc)
    for k, v in d.items():
        assert v <= PARITY_BOUND[k], "truncation mmax %d %s: %s %.3e beyond %.1e" % (mmax, trunc, k, v, PARITY_BOUND[k])


def check_window_matters(lib):
    """on the reference alone: mmax 1 and mmax 30 part by far more than the parity bound, so that a library that ignored
    the window could not pass check_truncation"""
    a, c = trunc_reference(lib, 1, "notay"), trunc_reference(lib, 30, "notay")
    gap = float(np.max(np.abs(a["hist"] - c["hist"])) / c["hist"][0])
    print("truncation: the histories of mmax 1 and mmax 30 differ by %.3e (bound %.1e)" % (gap, PARITY_BOUND["hist"]))
    assert gap > 1000.0 * PARITY_BOUND["hist"], gap


# ---------------------------------------------------------------------------------------------- fcg equals cg
def measure_equals_cg(lib, lvl, n, guess):
    """a fixed symmetric preconditioner: every window gives the direction of cg.  The inputs are those of the case
    (preconditioned norm), checked on the history of the library's cg."""
    pc = U.get_pc(lib, n, argv_for(lvl, CHEB))
    seed, rtol = SEEDS[(lvl, n, guess, "preconditioned")]
    b, x0 = rhs(n, seed)
    cg = run(pc, "cg", guess, b, x0, rtol)
    bad = input_ok(cg["hist"], cg["its"], threshold(pc, b, guess, "preconditioned", cg["hist"][0], rtol))
    out = {}
    for mmax in (1, 30):
        got = run(pc, "fcg", guess, b, x0, rtol, mmax=mmax)
        out[mmax] = (got["its"], float(np.max(np.abs(got["hist"][:min(len(got["hist"]), len(cg["hist"]))] -
                                                     cg["hist"][:min(len(got["hist"]), len(cg["hist"]))])) / cg["hist"][0]))
        print("fcg(%2d) against cg, %-8s %d^3 guess %d: its %d against %d, hist %.3e" % (
            mmax, lvl, n, guess, got["its"], cg["its"], out[mmax][1]))
    return cg, bad, out


def check_equals_cg(lib, lvl, n, guess):
    cg, bad, out = measure_equals_cg(lib, lvl, n, guess)
    assert cg["reason"] == "KSP_CONVERGED_RTOL" and bad is None, "bad input %s %d^3 guess %d: %s: pick another seed" % (lvl, n, guess, bad)
    for mmax, (its, dh) in out.items():
        assert its == cg["its"], "fcg(%d) %s: %d iterations, cg %d" % (mmax, lvl, its, cg["its"])
        assert dh <= PARITY_BOUND["hist"], "fcg(%d) against cg, %s: histories differ by %.3e" % (mmax, lvl, dh)


# ---------------------------------------------------------------------------------------------- a changing preconditioner
def check_nonlinear(lib, lvl, n, seed=7, rtol=1e-8):
    """-dls1_ksp_type cg -dls1_ksp_rtol 1e-2: every application of the preconditioner is another operator.  fcg converges in
    the true residual, which its recurrence r -= alpha A p follows whatever z was."""
    pc = U.get_pc(lib, n, argv_for(lvl, ["-dls1_ksp_type", "cg", "-dls1_ksp_rtol", "1e-2"]))
    a = U.grid(n)[2]
    b, x0 = rhs(n, seed)
    got = run(pc, "fcg", 0, b, x0, rtol, norm="unpreconditioned")
    cg = run(pc, "cg", 0, b, x0, rtol)
    true = float(np.linalg.norm(b - a @ got["x"]))
    nb = float(np.linalg.norm(b))
    print("fcg, -dls1_ksp_rtol 1e-2, %s %d^3: its %d (%s), rnorm %.3e, |b - A x| %.3e, |b| %.3e; cg on the same set-up: its %d (%s)" % (
        lvl, n, got["its"], got["reason"], got["rnorm"], true, nb, cg["its"], cg["reason"]))
    assert got["reason"].startswith("KSP_CONVERGED"), got["reason"]
    assert true <= max(rtol * nb, 1e-50) + PARITY_BOUND["rnorm"] * nb, (true, rtol * nb)
    return got


# ---------------------------------------------------------------------------------------------- counters
def check_counters(lib, lvl="ASM,1", n=12, on_gpu=False):
    """what the method holds and which form of the step ran -- on a PC of its own, so that nothing is shared"""
    import cases
    mesh, dec, a, _ = U.grid(n)
    ref = reference_for(lib, lvl, n, 0, "preconditioned")
    b, x0, rtol = ref["b"], ref["x0"], ref["rtol"]
    pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
    zero_k = pc.krylov_info()
    assert pc.fcg_info() == dict(directions=0, bytes=0.0, steps_fused=0, steps_composed=0, max_window=0, downloads=0), pc.fcg_info()
    cg = run(pc, "cg", 0, b, x0, rtol)                                   # another method allocates nothing for fcg
    assert cg["fcg"]["directions"] == 0 and cg["fcg"]["bytes"] == 0.0, cg["fcg"]
    total = dict(fused=0, composed=0)
    for mmax in (30, 3):
        got = run(pc, "fcg", 0, b, x0, rtol, mmax=mmax)
        its = got["its"]
        assert its == ref["its"] and its > 3 + 1
        total["fused" if on_gpu else "composed"] += its
        f = got["fcg"]
        assert f["steps_fused"] == total["fused"] and f["steps_composed"] == total["composed"], (f, total)
        # one download per iterate (its + 1); the composed step downloads S once more per step
        assert f["downloads"] == (its + 1 if on_gpu else 2 * its + 1), (f, its)
        # the window's mmax directions and the new one are alive together: the ring holds mmax + 1 pairs
        assert f["directions"] == min(its, mmax + 1), (f, its, mmax)
        assert f["max_window"] == max_window(its, mmax, "notay") == min(its - 1, mmax)
        assert f["bytes"] >= 8.0 * (2 * f["directions"] + 1) * mesh.nbNode
        assert got["info"]["pc_applies"] == its + 1 and got["info"]["mat_mults"] == its, got["info"]
        kept = {k: v for k, v in got["info"].items() if k not in ("pc_applies", "mat_mults")}
        assert kept == {k: v for k, v in zero_k.items() if k in kept}, "an fcg solve shows in PCGenEOGetKrylovInfo: %s" % (got["info"],)
    if on_gpu:
        with K.krylov_fused_off(lib):
            again = run(pc, "fcg", 0, b, x0, rtol, mmax=3)
        assert again["its"] == its
        assert again["fcg"]["steps_fused"] == total["fused"] and again["fcg"]["steps_composed"] == its, again["fcg"]
        assert again["fcg"]["downloads"] == 2 * its + 1, again["fcg"]
        assert np.linalg.norm(again["x"] - got["x"]) <= PARITY_BOUND["x"] * np.linalg.norm(got["x"])
    un = run(pc, "fcg", 0, b, x0, rtol, norm="unpreconditioned")
    assert un["info"]["pc_applies"] == un["its"] and un["info"]["mat_mults"] == un["its"], un["info"]
    pc.destroy()


def check_disturbs_nothing(lib, lvl, n, seed=11):
    """cg and left gmres before and after an fcg solve on the same PC, and on a fresh PC: the same counts and bits"""
    import cases
    mesh, dec, a, _ = U.grid(n)
    b, x0 = rhs(n, seed)
    methods = ("gmres", "cg")
    pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
    before = {m: run(pc, m, 1, b, x0, 1e-8) for m in methods}
    for norm in ("preconditioned", "unpreconditioned"):
        assert run(pc, "fcg", 1, b, x0, 1e-8, norm=norm)["reason"].startswith("KSP_CONVERGED")
    assert pc.fcg_info()["directions"] > 0
    after = {m: run(pc, m, 1, b, x0, 1e-8) for m in methods}
    pc.destroy()
    fresh_pc = cases.run_pc(lib, mesh, dec, argv_for(lvl, CHEB), b)
    fresh = {}
    for m in methods:
        K.set_method(fresh_pc, m, 30, 1)                                 # the options of a PC that never heard of fcg
        fresh_pc.set_option("-ksp_rtol", repr(1e-8))
        x, its, rnorm, reason = fresh_pc.solve(b, x0=x0.copy())
        fresh[m] = dict(x=x, its=its, reason=reason, hist=fresh_pc.residual_history().copy())
    assert fresh_pc.fcg_info()["directions"] == 0
    fresh_pc.destroy()
    for m in methods:
        for other, what in ((after[m], "after an fcg solve"), (fresh[m], "on a fresh PC")):
            assert before[m]["its"] == other["its"] and before[m]["reason"] == other["reason"], (m, what)
            assert same_bits(before[m]["hist"], other["hist"]) and same_bits(before[m]["x"], other["x"]), \
                "%s %s: not the same bits" % (m, what)
        assert before[m]["reason"].startswith("KSP_CONVERGED")
