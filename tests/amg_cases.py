"""The multigrid hierarchy and its V-cycle (csrc/amg.cpp) against a reference in np.longdouble: shared by
test_amg_vcycle_host.py (host twin, -m "not gpu") and test_gpu_amg_vcycle.py (-m gpu).

The hierarchy is created through the GeneoTestAmg* hooks of the C ABI and read back level by level.  The reference of
the cycle is the textbook recursion on the DOWNLOADED level matrices, dinv and rho (so it isolates AmgDevice::cycle from
the set-up; the set-up is checked against scipy separately, `identity_errors`):

    pre-smoothing from a zero guess, r = b - A x, e = V_{l+1}(R r), x += P e, post-smoothing from x
    smoothing = the Chebyshev-Jacobi recurrence of AmgDevice::smooth (degree 1: x += w D^-1 (b - A x),
    w = 1 / (0.5 (lmax + lmin)), lmax = 1.1 rho, lmin = lmax / max(1.5, ratio)); coarsest level: the dense inverses.

It is never written in the collapsed form x = w D^-1 (b + r1) + M e: that the M form, the two-launch form and the unfused
form equal the plain recursion is what the tests establish.  One exception, by necessity: the float-rounded reference of
a `single` hierarchy at m = 1 must round the entries the kernels read, and float32(M_ij) is not expressible through
float32(P_ij) and float32(A_ij); there, and only there, a level with M is evaluated through the rounded M (and the
zero-guess sweep through the rounded Acs = A diag(dinv)), every other matrix that reports a companion rounded likewise.

Matrix: block diagonal and SPD, four 7-point blocks with random edge coefficients in [0.5, 1.5] and a mass term;
12x11x10 (1320 rows, mass 2.0), 7x6x5 (210), 9x9x9 (729, coefficients x 1e3 in its lower half) and 3x3x2 (18), mass 0.05
each: 2277 rows, no block boundary a multiple of 64, the last block below coarse_size = 30 from the start.  The mass
terms give the blocks visibly different Gershgorin bounds (1.80 for the first, 2.00 for the third), so the per-subdomain
rescaling of dinv is at work; the sizes are the smallest at which the two large blocks pass through three levels.

Bounds.  Error measure of a block: max_j ||X_j - Xref_j||_inf / ||Xref_j||_inf.  The same numpy recursion evaluated in
float64 and in longdouble on these inputs (host twin hierarchies, all cases and applications of the host test file)
differs by at most
    REF_ROUNDING = 2.0e-15     (measured 1.98e-15, at max_levels = 1 and m = 32 where the cycle is the 1320 x 1320 dense
                                inverse alone; 9.5e-16 over the multilevel cases)
and the bound of every cycle comparison is 100 times that, the project's margin where only summation orders differ
(PARITY_BOUND in block_rhs_util.py):
    CYCLE_BOUND = 2.0e-13
The host tests re-measure the figure on every case and print it (numpy's float64 summation order, and with it the exact
figure, may differ between CPUs; they assert that it stays an order of magnitude under the bound).
The matrix identities are bounded the same way: scipy's float64 product against the longdouble evaluation of the same
product, entry-wise max |difference| / max |entry|, floored at one unit roundoff 2^-53, times 100 (`identity_errors`
returns the measured reference figure next to the code's, so the bound travels with the data).  The coarsest inverses
are bounded by 100 times the residual max |inv(A_s) A_s - I| of np.linalg.inv on the same block.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from geneo4petsc_amd import _lib as L

LD = np.longdouble
REF_ROUNDING = 2.0e-15
CYCLE_BOUND = 100 * REF_ROUNDING
U = 2.0 ** -53
SENT = -7.25e+97                 # prefill of X: padding columns must come back with these bits

BLOCKS = ((12, 11, 10), (7, 6, 5), (9, 9, 9), (3, 3, 2))
JUMP_BLOCK = 2
MASS = (2.0, 0.05, 0.05, 0.05)
COARSE_SIZE = 30
MAX_M = 32
MATRICES = ("A", "P", "R", "M", "Acs")

# (level, m, ldb, ldx): contiguous vector; a vector on the block path; blocks with both leading dimensions off m (16: the
# narrow SpMM, 20: no multiple of the tile, 32: the widest; an odd leading dimension keeps the top level off the sliced
# block kernel, so 16 and 32 run with even ones as well, which is how LOBPCG calls the cycle); the cycle from level 1 down
APPLIES = ((0, 1, 1, 1), (0, 1, 1, 3), (0, 16, 19, 96), (0, 20, 23, 96), (0, 32, 35, 96), (0, 16, 18, 96), (0, 32, 34, 96),
           (1, 1, 1, 1), (1, 16, 19, 96))


# ---- the matrix -----------------------------------------------------------------------------------------------------
def stencil_block(shape, rng, jump=False, mass=0.05):
    nx, ny, nz = shape
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    rows, cols, vals = [], [], []
    diag = np.full(idx.size, mass)
    for ax in range(3):
        lo = np.moveaxis(idx, ax, 0)[:-1].ravel()
        hi = np.moveaxis(idx, ax, 0)[1:].ravel()
        c = rng.uniform(0.5, 1.5, lo.size)
        if jump:
            c = np.where(np.unravel_index(lo, shape)[0] < nx // 2, 1e3 * c, c)
        np.add.at(diag, lo, c)
        np.add.at(diag, hi, c)
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-c, -c]
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append(diag)
    a = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(idx.size, idx.size)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def make_blocks(seed=20240607):
    rng = np.random.default_rng(seed)
    return [stencil_block(s, rng, jump=(i == JUMP_BLOCK), mass=MASS[i]) for i, s in enumerate(BLOCKS)]


def batch_of(blocks):
    a = sp.block_diag(blocks, format="csr")
    a.sort_indices()
    suboff = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int32)
    return a, suboff


# ---- the hook -------------------------------------------------------------------------------------------------------
class Csr:
    """CSR arrays as downloaded (entry order and structural zeros kept)"""

    def __init__(self, n, ncols, rowptr, col, val):
        self.n, self.ncols, self.rowptr, self.col, self.val = n, ncols, rowptr, col, val

    def sp(self):
        return sp.csr_matrix((self.val, self.col, self.rowptr), shape=(self.n, self.ncols))


class Level:
    pass


def _ip(a):
    return a.ctypes.data_as(L.c_int_p)


def _dp(a):
    return a.ctypes.data_as(L.c_dbl_p)


def err_text(lib):
    return lib.PCGenEOGetError(None).decode()


class Hierarchy:
    """setup: "device" (build_on_device; raises if it declines) | "host" (amg_setup_host + upload)"""

    def __init__(self, lib, a, suboff, setup="device", degree=1, ratio=4.0, strength=0.0, max_levels=10, single=False,
                 fine_companion=False, coarse_size=COARSE_SIZE, max_m=MAX_M):
        self.lib, self.degree, self.ratio, self.single = lib, degree, ratio, single
        a = a.tocsr()
        rp, col, val = a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)
        suboff = np.ascontiguousarray(suboff, dtype=np.int32)
        g = L.GeneoCsr(a.shape[0], _ip(rp), _ip(col), _dp(val))
        ipar = np.array([coarse_size, degree, max_levels, int(single), max_m, {"device": 0, "host": 1}[setup],
                         int(fine_companion)], dtype=np.int32)
        dpar = np.array([ratio, strength])
        self.h = C.c_void_p()
        rc = lib.GeneoTestAmgCreate(C.byref(g), len(suboff) - 1, _ip(suboff), _ip(ipar), _dp(dpar), C.byref(self.h))
        assert rc != 2, "the device set-up declined (a row beyond the product kernels' capacity)"
        assert rc == 0, err_text(lib)
        try:
            self._read(len(suboff) - 1)
        except BaseException:
            self.destroy()
            raise

    def _read(self, nsub):
        lib = self.lib
        nl, opc, nlp = C.c_int(), C.c_double(), C.c_int()
        assert lib.GeneoTestAmgInfo(self.h, C.byref(nl), C.byref(opc), C.byref(nlp)) == 0
        self.nlevels, self.opc, self.lp_matrices = nl.value, opc.value, nlp.value
        self.levels = [self._level(l) for l in range(self.nlevels)]
        for l, lv in enumerate(self.levels):                    # the column counts come from the neighbours
            nc = self.levels[l + 1].n if l + 1 < self.nlevels else 0
            lv.A.ncols = lv.n
            if lv.Acs is not None:
                lv.Acs.ncols = lv.n
            for m in (lv.P, lv.M):
                if m is not None:
                    m.ncols = nc
            if lv.R is not None:
                lv.R.ncols = lv.n
        base = np.zeros(nsub + 1, dtype=np.int64)
        tot = lib.GeneoTestAmgCoarseInverse(self.h, base.ctypes.data_as(C.POINTER(C.c_longlong)), None, 0)
        assert tot >= 0, err_text(lib)
        self.cinv = np.zeros(max(1, tot))
        assert lib.GeneoTestAmgCoarseInverse(self.h, base.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(self.cinv), tot) == tot
        self.cbase = base

    def _level(self, l):
        lib = self.lib
        io = np.zeros(11, dtype=np.int64)
        rho = C.c_double()
        assert lib.GeneoTestAmgLevel(self.h, l, io.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(rho), None, None) == 0, err_text(lib)
        lv = Level()
        lv.n, lv.nsub, lv.fused, lv.vec_lpr, lv.nlong = int(io[0]), int(io[1]), int(io[2]), int(io[3]), int(io[4])
        lv.rho = rho.value
        lv.suboff = np.zeros(lv.nsub + 1, dtype=np.int32)
        lv.dinv = np.zeros(lv.n)
        assert lib.GeneoTestAmgLevel(self.h, l, None, None, _ip(lv.suboff), _dp(lv.dinv)) == 0, err_text(lib)
        lv.lp = {}
        for w, name in enumerate(MATRICES):
            nnz = int(io[6 + w])
            lv.lp[name] = bool(io[5] >> w & 1)
            if nnz < 0:
                setattr(lv, name, None)
                continue
            rows = C.c_int()
            rp, col, val = np.zeros(0, np.int32), np.zeros(max(1, nnz), np.int32), np.zeros(max(1, nnz))
            assert lib.GeneoTestAmgMatrix(self.h, l, w, C.byref(rows), None, None, None, 0) == nnz
            rp = np.zeros(rows.value + 1, np.int32)
            assert lib.GeneoTestAmgMatrix(self.h, l, w, C.byref(rows), _ip(rp), _ip(col), _dp(val), nnz) == nnz, err_text(lib)
            assert rp[0] == 0 and rp[-1] == nnz
            setattr(lv, name, Csr(rows.value, 0, rp, col[:nnz], val[:nnz]))
        return lv

    def vcycle(self, level, B, X, m):
        """B (n x ldb), X (n x ldx) C-contiguous float64, both in place: what the device left in them"""
        assert B.flags.c_contiguous and X.flags.c_contiguous and B.dtype == np.float64 and X.dtype == np.float64
        assert B.shape[0] == X.shape[0] == self.levels[level].n
        rc = self.lib.GeneoTestAmgVcycle(self.h, level, _dp(B), B.shape[1], _dp(X), X.shape[1], m)
        assert rc == 0, err_text(self.lib)

    def destroy(self):
        if self.h:
            assert self.lib.GeneoTestAmgDestroy(C.byref(self.h)) == 0


# ---- the reference --------------------------------------------------------------------------------------------------
def csr_mm(m, X, dt, rounded=False):
    """m @ X in dt by segment sums over the stored entries (empty rows: zero); rounded: the entries through float32"""
    v = m.val.astype(np.float32).astype(dt) if rounded else m.val.astype(dt)
    out = np.zeros((m.n, X.shape[1]), dt)
    rows = np.flatnonzero(m.rowptr[1:] > m.rowptr[:-1])
    if rows.size:
        out[rows] = np.add.reduceat(v[:, None] * X[m.col], m.rowptr[:-1][rows], axis=0)
    return out


def smoother_scalars(rho, ratio):
    lmax = 1.1 * rho
    lmin = lmax / max(1.5, ratio)
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    return theta, delta, theta / delta


def jacobi_weight(rho, ratio):
    return 1.0 / smoother_scalars(rho, ratio)[0]


def ref_smooth(lv, B, X, degree, ratio, dt, mm):
    """AmgDevice::smooth: X None = zero guess"""
    theta, delta, sigma = smoother_scalars(lv.rho, ratio)
    dinv = lv.dinv.astype(dt)[:, None]
    r = B.copy() if X is None else B - mm("A", X)
    d = dt(1.0 / theta) * dinv * r
    X = d.copy() if X is None else X + d
    rho = 1.0 / sigma
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        r = r - mm("A", d)
        d = dt(2.0 * rho_new / delta) * dinv * r + dt(rho_new * rho) * d
        X = X + d
        rho = rho_new
    return X


def ref_vcycle(H, level, B, dt, rounded=False):
    """V_level(B), B n x m.  rounded: the storage a `single` hierarchy reads at m = 1 (module docstring)"""
    lv = H.levels[level]
    B = B.astype(dt)
    if level == H.nlevels - 1:
        X = np.zeros_like(B)
        so = lv.suboff
        for s in range(lv.nsub):
            ns = so[s + 1] - so[s]
            inv = H.cinv[H.cbase[s]:H.cbase[s + 1]].reshape(ns, ns).astype(dt)
            X[so[s]:so[s + 1]] = inv @ B[so[s]:so[s + 1]]
        return X

    # the companions are read by the fused damped-Jacobi branch alone: every other level applies its FP64 matrices
    lp_level = rounded and H.degree <= 1 and lv.fused

    def mm(name, V):
        return csr_mm(getattr(lv, name), V, dt, lp_level and lv.lp[name])

    if lp_level:
        w = dt(jacobi_weight(lv.rho, H.ratio))
        dinv = lv.dinv.astype(dt)[:, None]
        x1 = w * dinv * B
        r1 = B - (mm("Acs", w * B) if lv.Acs is not None else mm("A", x1))
        e = ref_vcycle(H, level + 1, mm("R", r1), dt, rounded)
        if lv.M is not None:
            return w * dinv * (B + r1) + mm("M", e)
        t = x1 + mm("P", e)
        return t + w * dinv * (B - mm("A", t))
    X = ref_smooth(lv, B, None, H.degree, H.ratio, dt, mm)
    r = B - mm("A", X)
    e = ref_vcycle(H, level + 1, mm("R", r), dt, rounded)
    X = X + mm("P", e)
    return ref_smooth(lv, B, X, H.degree, H.ratio, dt, mm)


def rel_err(X, Xref):
    X, Xref = np.asarray(X, LD), np.asarray(Xref, LD)
    return float(np.max(np.abs(X - Xref).max(axis=0) / np.abs(Xref).max(axis=0)))


def apply_and_compare(H, level, m, ldb, ldx, seed, rounded=False):
    """One application of the cycle: asserts the padding of X and the bits of B, returns (error against the longdouble
    reference, error of the float64 evaluation of the reference against it)."""
    n = H.levels[level].n
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, ldb))
    X = np.full((n, ldx), SENT)
    B0 = B.copy()
    H.vcycle(level, B, X, m)
    assert B.tobytes() == B0.tobytes(), "the cycle changed its right-hand side"
    assert np.all(X[:, m:].view(np.int64) == np.float64(SENT).view(np.int64)), "the cycle wrote into the padding of X"
    assert np.all(np.isfinite(X[:, :m]))
    ref = ref_vcycle(H, level, B0[:, :m], LD, rounded)
    ref64 = ref_vcycle(H, level, B0[:, :m], np.float64, rounded)
    return rel_err(X[:, :m], ref), rel_err(ref64, ref)


# ---- the cycle: cases -----------------------------------------------------------------------------------------------
# name -> (environment, Hierarchy arguments, expectations on the reported flags)
CYCLE_CASES = {
    "device-default": ({}, dict(setup="device"), ("has_M", "has_Acs", "fused", "deep")),
    "device-no-post-matrix": ({"GENEO_AMG_NO_POST_MATRIX": "1"}, dict(setup="device"), ("no_M", "has_Acs", "fused")),
    "device-no-prescale": ({"GENEO_AMG_NO_PRESCALE": "1"}, dict(setup="device"), ("has_M", "no_Acs", "fused")),
    "device-unfused": ({"GENEO_AMG_UNFUSED": "1"}, dict(setup="device"), ("unfused", "no_M")),
    "device-degree2": ({}, dict(setup="device", degree=2), ("no_M", "deep")),
    "device-degree3": ({}, dict(setup="device", degree=3), ("no_M",)),
    "device-max-levels-1": ({}, dict(setup="device", max_levels=1), ("levels1",)),
    "device-max-levels-2": ({}, dict(setup="device", max_levels=2), ("levels2", "has_M")),
    "host-default": ({}, dict(setup="host"), ("has_M", "has_Acs", "fused", "deep")),
    "host-degree2": ({}, dict(setup="host", degree=2), ("no_M", "deep")),
    "host-upload-r-default": ({"GENEO_AMG_UPLOAD_R": "1"}, dict(setup="host"), ("has_M", "fused", "deep")),
    "host-upload-r-degree2": ({"GENEO_AMG_UPLOAD_R": "1"}, dict(setup="host", degree=2), ("no_M", "deep")),
}
AMG_ENV = ("GENEO_AMG_NO_POST_MATRIX", "GENEO_AMG_NO_PRESCALE", "GENEO_AMG_UNFUSED", "GENEO_AMG_UPLOAD_R", "GENEO_AMG_HOST",
           "GENEO_AMG_SHARED_RHO", "GENEO_AGG_THREADS", "GENEO_AGG_MIN_NNZ")


def set_env(monkeypatch, env):
    for k in AMG_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_flags(H, expect):
    """the case reached the branch it is named for"""
    inner = H.levels[:-1]
    for e in expect:
        if e == "has_M":
            assert any(lv.M is not None for lv in inner)
        elif e == "no_M":
            assert inner and all(lv.M is None for lv in inner)
        elif e == "has_Acs":
            assert any(lv.Acs is not None for lv in inner)
        elif e == "no_Acs":
            assert inner and all(lv.Acs is None for lv in inner)
        elif e == "fused":
            assert inner and all(lv.fused for lv in inner)
        elif e == "unfused":
            assert all(not lv.fused for lv in H.levels)
        elif e == "deep":
            assert H.nlevels >= 3
        elif e == "levels1":
            assert H.nlevels == 1
        elif e == "levels2":
            assert H.nlevels == 2
        else:
            raise KeyError(e)


def run_cycle_case(lib, monkeypatch, name, a, suboff, tag):
    """Builds the hierarchy of a case, checks its flags, applies every form of APPLIES; prints and returns the largest
    (error, float64 reference error)."""
    env, kw, expect = CYCLE_CASES[name]
    set_env(monkeypatch, env)
    H = Hierarchy(lib, a, suboff, **kw)
    try:
        check_flags(H, expect)
        worst, worst64 = 0.0, 0.0
        for i, (level, m, ldb, ldx) in enumerate(APPLIES):
            if level >= H.nlevels:
                continue
            err, err64 = apply_and_compare(H, level, m, ldb, ldx, seed=100 + i)
            print("amg-cycle %s %s levels=%d from=%d m=%d ldb=%d ldx=%d err=%.2e ref64=%.2e bound=%.1e"
                  % (tag, name, H.nlevels, level, m, ldb, ldx, err, err64, CYCLE_BOUND))
            worst, worst64 = max(worst, err), max(worst64, err64)
        return H.nlevels, worst, worst64, [lv.vec_lpr for lv in H.levels]
    finally:
        H.destroy()


# ---- the hierarchy against scipy ------------------------------------------------------------------------------------
def _dense(m, dt=LD):
    out = np.zeros((m.n, m.ncols), dt)
    np.add.at(out, (np.repeat(np.arange(m.n), np.diff(m.rowptr)), m.col), m.val.astype(dt))
    return out


def _mat_err(x, ref):
    ref = np.asarray(ref, LD)
    return float(np.abs(np.asarray(x, LD) - ref).max() / np.abs(ref).max())


def gershgorin(a, suboff, dt):
    """(rho, dinv) of amg.cpp's gershgorin_rho evaluated in dt: per block rho_s = max_i sum_j |a_ij| / a_ii, rho their
    maximum, dinv_i = (rho / rho_s) / a_ii"""
    a = a.tocsr()
    d = a.diagonal().astype(dt)
    rowsum = np.add.reduceat(np.abs(a.data.astype(dt)), a.indptr[:-1])
    q = rowsum / d
    rho_s = np.array([q[suboff[s]:suboff[s + 1]].max() for s in range(len(suboff) - 1)], dtype=dt)
    rho = rho_s.max()
    dinv = dt(1.0) / d
    for s in range(len(suboff) - 1):
        if rho_s[s] != rho:
            dinv[suboff[s]:suboff[s + 1]] *= rho / rho_s[s]
    return rho, dinv, rho_s


def identity_errors(H, a0):
    """name -> (figure of the hierarchy, figure of the float64 reference evaluation) for the set-up identities that carry
    a rounding error; the exact ones (R = P^T, block structure, complexity) are asserted here."""
    out = {}
    nnz = []
    for l, lv in enumerate(H.levels):
        A = lv.A
        assert A.n == lv.n and lv.suboff[0] == 0 and lv.suboff[-1] == lv.n
        nnz.append(len(A.val))
        As = A.sp()
        # dinv and rho
        rho_ld, dinv_ld, _ = gershgorin(As, lv.suboff, LD)
        rho_64, dinv_64, _ = gershgorin(As, lv.suboff, np.float64)
        out["rho[%d]" % l] = (abs(float((LD(lv.rho) - rho_ld) / rho_ld)), abs(float((LD(rho_64) - rho_ld) / rho_ld)))
        out["dinv[%d]" % l] = (float(np.abs((lv.dinv.astype(LD) - dinv_ld) / dinv_ld).max()),
                               float(np.abs((dinv_64.astype(LD) - dinv_ld) / dinv_ld).max()))
        if l + 1 == H.nlevels:
            assert lv.P is None and lv.R is None and lv.M is None
            break
        nxt = H.levels[l + 1]
        P, R = lv.P, lv.R
        assert P.n == lv.n and R.n == nxt.n
        # R = P^T: same pattern, same bits
        Pt = P.sp().T.tocsr()
        Rs = R.sp()
        Pt.sort_indices()
        Rs.sort_indices()
        assert np.array_equal(Pt.indptr, Rs.indptr) and np.array_equal(Pt.indices, Rs.indices), "pattern of R at level %d" % l
        assert Pt.data.tobytes() == Rs.data.tobytes(), "bits of R at level %d" % l
        # P is block diagonal with respect to suboff_l x suboff_{l+1}
        prow = np.repeat(np.arange(P.n), np.diff(P.rowptr))
        rs = np.searchsorted(lv.suboff, prow, side="right") - 1
        assert np.all((nxt.suboff[rs] <= P.col) & (P.col < nxt.suboff[rs + 1])), "P couples two subdomains at level %d" % l
        # P 1 = (I - 4 / (3 rho) D^-1 A) 1
        one = np.ones((lv.n, 1))
        onec = np.ones((nxt.n, 1))
        ref = one.astype(LD) - LD(4.0 / (3.0 * lv.rho)) * lv.dinv.astype(LD)[:, None] * csr_mm(A, one.astype(LD), LD)
        ref64 = one - (4.0 / (3.0 * lv.rho)) * lv.dinv[:, None] * (As @ one)
        out["P1[%d]" % l] = (_mat_err(csr_mm(P, onec.astype(LD), LD), ref), _mat_err(ref64, ref))
        # Galerkin product and post-smoothing matrix
        Pd = _dense(P)
        AP = csr_mm(A, Pd, LD)
        RAP = csr_mm(R, AP, LD)
        RAP64 = (Rs @ As @ P.sp()).toarray()
        out["RAP[%d]" % l] = (_mat_err(_dense(nxt.A), RAP), _mat_err(RAP64, RAP))
        if lv.M is not None:
            w = jacobi_weight(lv.rho, H.ratio)
            Mref = Pd - LD(w) * lv.dinv.astype(LD)[:, None] * AP
            M64 = (P.sp() - sp.diags(w * lv.dinv) @ As @ P.sp()).toarray()
            out["M[%d]" % l] = (_mat_err(_dense(lv.M), Mref), _mat_err(M64, Mref))
        if lv.Acs is not None:
            assert np.array_equal(lv.Acs.rowptr, A.rowptr) and np.array_equal(lv.Acs.col, A.col)
            ref = A.val.astype(LD) * lv.dinv.astype(LD)[A.col]
            out["Acs[%d]" % l] = (float(np.abs((lv.Acs.val.astype(LD) - ref) / ref).max()),
                                  float(np.abs(((A.val * lv.dinv[A.col]).astype(LD) - ref) / ref).max()))
    # level 0 is the caller's matrix, bit for bit
    a0 = a0.tocsr()
    assert np.array_equal(H.levels[0].A.rowptr, a0.indptr) and np.array_equal(H.levels[0].A.col, a0.indices)
    assert H.levels[0].A.val.tobytes() == a0.data.astype(np.float64).tobytes()
    assert H.opc == sum(nnz) / nnz[0], (H.opc, sum(nnz) / nnz[0])
    # coarsest inverses
    last = H.levels[-1]
    Ad = last.A.sp().toarray()
    worst, worst_ref = 0.0, 0.0
    for s in range(last.nsub):
        r0, r1 = last.suboff[s], last.suboff[s + 1]
        if r1 == r0:
            continue
        blk = Ad[r0:r1, r0:r1]
        assert H.cbase[s + 1] - H.cbase[s] == (r1 - r0) ** 2
        inv = H.cinv[H.cbase[s]:H.cbase[s + 1]].reshape(r1 - r0, r1 - r0)
        eye = np.eye(r1 - r0)
        worst = max(worst, float(np.abs(inv.astype(LD) @ blk.astype(LD) - eye).max()))
        worst_ref = max(worst_ref, float(np.abs(np.linalg.inv(blk).astype(LD) @ blk.astype(LD) - eye).max()))
    out["coarse_inverse"] = (worst, worst_ref)
    return out


def assert_identities(H, a0, tag):
    errs = identity_errors(H, a0)
    bad = []
    for name, (got, ref) in errs.items():
        bound = 100 * max(ref, U)
        print("amg-setup %s %s err=%.2e reference=%.2e bound=%.1e" % (tag, name, got, ref, bound))
        if not got <= bound:
            bad.append((name, got, bound))
    assert not bad, bad
    return errs


def assert_same_hierarchy(Hd, Hh, a0, tag):
    """device set-up against host set-up: sizes and offsets equal, matrices equal as values (structural zeros may differ).
    The two set-ups evaluate the same products in different orders, so they may differ by what one float64 evaluation of
    those products differs from the exact one: the bound is 100 x the largest float64-against-longdouble figure of the
    set-up identities on the host hierarchy (`identity_errors`; the coarsest inverses, a different operation, left out)."""
    ref = max(r for name, (_, r) in identity_errors(Hh, a0).items() if name != "coarse_inverse")
    bound = 100 * max(ref, U)
    assert Hd.nlevels == Hh.nlevels
    for l, (d, h) in enumerate(zip(Hd.levels, Hh.levels)):
        assert d.n == h.n and np.array_equal(d.suboff, h.suboff), l
        for name in ("A", "P", "R"):
            md, mh = getattr(d, name), getattr(h, name)
            assert (md is None) == (mh is None), (l, name)
            if md is None:
                continue
            err = _mat_err(md.sp().toarray(), mh.sp().toarray())
            print("amg-setup %s device-vs-host %s[%d] err=%.2e reference=%.2e bound=%.1e" % (tag, name, l, err, ref, bound))
            assert err <= bound, (l, name, err)
        assert abs(d.rho - h.rho) <= bound * h.rho
        assert np.abs(d.dinv - h.dinv).max() <= bound * np.abs(h.dinv).max()


# ---- independence from the batch ------------------------------------------------------------------------------------
ALONE_BLOCKS = (0, 2)     # the blocks that need the batch's depth on their own (a smaller block alone stops coarsening earlier)


def check_batch_independence(lib, blocks, batch, degree, tag):
    a, suboff = batch
    Hb = Hierarchy(lib, a, suboff, setup="device", degree=degree)
    rescaled = 1.0
    try:
        for s in ALONE_BLOCKS:
            n = blocks[s].shape[0]
            Ha = Hierarchy(lib, blocks[s], np.array([0, n], dtype=np.int32), setup="device", degree=degree)
            try:
                assert Ha.nlevels == Hb.nlevels
                r0 = suboff[s]
                assert np.array_equal(Ha.levels[1].suboff[1] - Ha.levels[1].suboff[0],
                                      Hb.levels[1].suboff[s + 1] - Hb.levels[1].suboff[s])     # same aggregates
                rescaled = min(rescaled, Ha.levels[0].rho / Hb.levels[0].rho)
                for i, (m, ldb, ldx) in enumerate(((1, 1, 1), (16, 19, 96))):
                    rng = np.random.default_rng(300 + 10 * s + i)
                    Bb = rng.standard_normal((a.shape[0], ldb))
                    Ba = np.ascontiguousarray(Bb[r0:r0 + n])
                    Xb, Xa = np.full((a.shape[0], ldx), SENT), np.full((n, ldx), SENT)
                    Hb.vcycle(0, Bb, Xb, m)
                    Ha.vcycle(0, Ba, Xa, m)
                    err = rel_err(Xb[r0:r0 + n, :m], Xa[:, :m])
                    ref = ref_vcycle(Ha, 0, Ba[:, :m], LD)
                    print("amg-batch %s degree=%d block=%d m=%d rho alone=%.6f batch=%.6f err=%.2e (alone against its reference %.2e) bound=%.1e"
                          % (tag, degree, s, m, Ha.levels[0].rho, Hb.levels[0].rho, err, rel_err(Xa[:, :m], ref), CYCLE_BOUND))
                    assert err <= CYCLE_BOUND
            finally:
                Ha.destroy()
        assert rescaled < 0.95        # a block whose own bound is visibly not the batch's: its dinv was rescaled there
    finally:
        Hb.destroy()
