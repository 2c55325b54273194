"""bk::spgemm and bk::transpose at every dispatch path and capacity edge, for any bound library (the cases are appended to
primitive_cases.CASES: test_gpu_primitives.py runs them on the HIP backend, test_hostsim_primitives.py on the host twin).

The cases are built around constants of csrc/backend_hip.hip, read from the source by regular expression and asserted
to be the values the cases were designed for (`constants`): a changed constant fails here instead of moving a case off
its edge.  The path of every row is computed on the host from the inputs (`classify`):
  grouped  k_spgemm_small<G>: na <= G entries in the row of A and at most G products (G from the average row, a.n >= 256)
  small64  wave per row, at most 64 products, na <= SPG_KMAX: sorted across the lanes, no hash table
  prefix   wave per row, hash table, product number -> (k, l) through the prefix table (na <= SPG_KMAX)
  serial   wave per row, hash table, rows of A longer than SPG_KMAX: entry by entry
and every case asserts that it holds the rows it was built to hold.  On the HIP backend the report of the product
(pc.sparse_product_report: group width, deferred rows, scan depth) must match what the host computed, and results over
the capacities must be None; the host twin has no capacities and reports zeros.

Checks of every spgemm case (`check_spgemm`), u = 2^-53:
  * exact data: entries are non-zero integers of -3 .. 3, so every product and partial sum is a small integer, exact in
    any order and under FMA contraction.  indptr, indices and the bits of data equal scipy's int64 product on the
    pattern of abs(A) @ abs(B): cancellations stay as stored zeros.
  * real data in (-0.5, 0.5) against the product evaluated in np.longdouble, entry by entry within
    (t + 2) u (|A| |B|)_ij, t the number of products of the entry (Higham, Accuracy and Stability, s. 3.1).
  * columns strictly increasing in every row; two runs give the same bits; the forms spgemm_fill_scan = 1 and
    spgemm_small_rows = 0 give the same bits as the default.
"""
import ctypes as C
import os
import re

import numpy as np
import scipy.sparse as sp

import geneo4petsc_amd
from geneo4petsc_amd import _lib as L
from geneo4petsc_amd.pc import _csr_struct, sparse_product_report

LD = np.longdouble
U = 2.0 ** -53
GROUPED, SMALL64, PREFIX, SERIAL = 0, 1, 2, 3
CLASS_NAMES = ("grouped", "small64", "prefix", "serial")
HASH_MUL = 2654435761
_I32 = np.int32


# ---------------------------------------------------------------------------------------------- constants of the source
class _K:
    pass


_consts = None


def constants():
    """the constants the cases are built around, from csrc/backend_hip.hip, asserted to be the designed values"""
    global _consts
    if _consts is not None:
        return _consts
    src = open(os.path.join(os.path.dirname(os.path.abspath(geneo4petsc_amd.__file__)), "csrc", "backend_hip.hip")).read()
    k = _K()
    for name in ("SPG_HS", "SPG_MAXD", "SPG_KMAX", "SPG_CHUNK", "TR_MAXROW", "SCAN_B"):
        m = re.findall(r"^constexpr int %s = (\d+);" % name, src, flags=re.M)
        assert len(m) == 1, "constexpr int %s: %d definitions" % (name, len(m))
        setattr(k, name, int(m[0]))
    m = re.findall(r"\(int64_t\)n < (\d+) \* SCAN_B", src)
    assert len(m) == 1, "threshold of the device scan in host_exclusive_scan: %r" % m
    k.SCAN_MIN = int(m[0]) * k.SCAN_B
    m = re.findall(r"a\.n >= (\d+) && b\.n > 0", src)
    assert len(m) == 1, "minimum row count of the group pass: %r" % m
    k.GROUP_MIN_ROWS = int(m[0])
    k.BANDS = [(float(a), float(e), int(g)) for a, e, g in re.findall(r"na <= ([\d.]+) && est <= ([\d.]+)\) G = (\d+);", src)]
    m = set(re.findall(r"total >= 0 && total <= (\d+) && !g_spgemm_no_small", src))
    assert len(m) == 1, "product count of the shuffle-sorted rows: %r" % m
    k.SMALL_MAX = int(m.pop())
    m = re.findall(r"constexpr int NB = (\d+); +// products per lane and round", src)
    assert len(m) == 1, "products per lane and round of the numeric pass: %r" % m
    k.ROUND = 64 * int(m[0])
    m = re.findall(r"\(unsigned\)key \* (\d+)u\) & \(SPG_HS - 1\)", src)
    assert m and set(m) == {str(HASH_MUL)}, "hash of the column sets: %r" % m
    got = dict(SPG_HS=k.SPG_HS, SPG_MAXD=k.SPG_MAXD, SPG_KMAX=k.SPG_KMAX, SPG_CHUNK=k.SPG_CHUNK, TR_MAXROW=k.TR_MAXROW,
               SCAN_B=k.SCAN_B, SCAN_MIN=k.SCAN_MIN, GROUP_MIN_ROWS=k.GROUP_MIN_ROWS, SMALL_MAX=k.SMALL_MAX, ROUND=k.ROUND,
               BANDS=k.BANDS)
    designed = dict(SPG_HS=512, SPG_MAXD=256, SPG_KMAX=256, SPG_CHUNK=256, TR_MAXROW=1024, SCAN_B=1024, SCAN_MIN=4096,
                    GROUP_MIN_ROWS=256, SMALL_MAX=64, ROUND=256,
                    BANDS=[(7.5, 7.5, 8), (15.0, 14.0, 16), (30.0, 26.0, 32), (60.0, 52.0, 64)])
    assert got == designed, "constants of backend_hip.hip moved away from the values these cases were built for: %r" % \
        {n: (got[n], designed[n]) for n in got if got[n] != designed[n]}
    _consts = k
    return k


def scan_depth(n):
    """depth of the row-pointer scan over n counts: 0 host loop, 1 one level of block totals, 2 totals in > 1 block"""
    k = constants()
    if n < k.SCAN_MIN:
        return 0
    return 2 if (n + k.SCAN_B - 1) // k.SCAN_B > k.SCAN_B else 1


def is_hip(lib):
    return lib.GeneoBackendName() == b"hip-gfx950"


# ---------------------------------------------------------------------------------------------- patterns and values
def pattern(rows, ncols):
    """CSR pattern (rowptr, col, ncols) from a list of column lists; every row strictly increasing"""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(_I32)
    col = np.concatenate([np.asarray(r, dtype=_I32).reshape(-1) for r in rows] + [np.zeros(0, dtype=_I32)])
    check_pattern(rp, col, ncols)
    return rp, col, int(ncols)


def check_pattern(rp, col, ncols):
    assert strictly_increasing(rp, col), "test bug: a row with unsorted or repeated columns"
    assert len(col) == 0 or (col.min() >= 0 and col.max() < ncols), "test bug: column out of range"


def strictly_increasing(rp, col):
    nnz = len(col)
    if nnz < 2:
        return True
    inner = np.ones(nnz - 1, dtype=bool)
    starts = np.asarray(rp[1:-1], dtype=np.int64)
    starts = starts[(starts > 0) & (starts < nnz)]
    inner[starts - 1] = False                               # differences across a row boundary do not count
    return bool((np.diff(col.astype(np.int64))[inner] > 0).all())


def values(nnz, kind, rng):
    if kind == "int":
        return rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=nnz)
    v = rng.random(nnz) - 0.5
    v[v == 0.0] = 0.25
    return v


def pick_group(pa, pb):
    """the group width spgemm takes for these operands (bands of the average row)"""
    k = constants()
    n, nb = len(pa[0]) - 1, len(pb[0]) - 1
    if n < k.GROUP_MIN_ROWS or nb <= 0:
        return 0
    na = float(pa[0][-1]) / n
    est = na * (float(pb[0][-1]) / nb)
    for amax, emax, g in k.BANDS:
        if na <= amax and est <= emax:
            return g
    return 0


def classify(pa, pb, group):
    """class of every row of A (GROUPED / SMALL64 / PREFIX / SERIAL), its entries and its products"""
    k = constants()
    arp, acol = pa[0].astype(np.int64), pa[1]
    n = len(arp) - 1
    na = np.diff(arp)
    blen = np.diff(pb[0].astype(np.int64))
    arow = np.repeat(np.arange(n), na)
    total = np.bincount(arow, weights=blen[acol], minlength=n).astype(np.int64)
    cls = np.where(na > k.SPG_KMAX, SERIAL, np.where(total <= k.SMALL_MAX, SMALL64, PREFIX))
    if group:
        cls[(na <= group) & (total <= group)] = GROUPED
    return cls, na, total


def class_counts(cls):
    return {CLASS_NAMES[c]: int((cls == c).sum()) for c in range(4)}


# ---------------------------------------------------------------------------------------------- references
def expand(pa, pb):
    """every product of A B in the order of the kernels (row, k, l): row of A, entry of A, entry of B"""
    arp, acol = pa[0].astype(np.int64), pa[1].astype(np.int64)
    brp = pb[0].astype(np.int64)
    n = len(arp) - 1
    rep = np.diff(brp)[acol]
    ent = np.repeat(np.arange(len(acol)), rep)
    first = np.cumsum(rep) - rep
    l = brp[acol][ent] + (np.arange(int(rep.sum())) - first[ent])
    arow = np.repeat(np.arange(n), np.diff(arp))
    return arow[ent], ent, l


class Reference:
    """pattern of A B (from the expanded products, the same as scipy's abs(A) @ abs(B)) and, per entry, its products"""

    def __init__(self, pa, pb):
        n, ncols = len(pa[0]) - 1, pb[2]
        self.n, self.ncols = n, ncols
        prow, self.ent, self.l = expand(pa, pb)
        key = prow * np.int64(ncols) + pb[1].astype(np.int64)[self.l]
        self.order = np.argsort(key, kind="stable")
        self.keys, self.start, self.count = np.unique(key[self.order], return_index=True, return_counts=True)
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(self.keys // ncols, minlength=n))]).astype(_I32)
        self.indices = (self.keys % ncols).astype(_I32)
        self.nnz = len(self.keys)
        one = lambda p: sp.csr_matrix((np.ones(len(p[1]), dtype=np.int64), p[1], p[0]), shape=(len(p[0]) - 1, p[2]))
        pat = (one(pa) @ one(pb)).tocsr()
        pat.sort_indices()
        assert (pat.indptr == self.indptr).all() and (pat.indices == self.indices).all(), "test bug: two reference patterns"

    def exact(self, pa, va, pb, vb):
        """scipy on int64, laid over the pattern with its zeros kept"""
        m = lambda p, v: sp.csr_matrix((v.astype(np.int64), p[1], p[0]), shape=(len(p[0]) - 1, p[2]))
        c = (m(pa, va) @ m(pb, vb)).tocsr()
        c.sort_indices()
        ckeys = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(c.indptr)) * np.int64(self.ncols) + c.indices
        at = np.searchsorted(self.keys, ckeys)
        assert (self.keys[at] == ckeys).all()
        out = np.zeros(self.nnz, dtype=np.int64)
        out[at] = c.data
        return out.astype(np.float64)

    def longdouble(self, va, vb):
        """(sums, sums of absolute products), both accumulated in longdouble"""
        if self.nnz == 0:
            return np.zeros(0, dtype=LD), np.zeros(0, dtype=LD)
        prod = (va[self.ent].astype(LD) * vb[self.l].astype(LD))[self.order]
        return np.add.reduceat(prod, self.start), np.add.reduceat(np.abs(prod), self.start)


# ---------------------------------------------------------------------------------------------- running a product
def _struct(p, v):
    arrs = (np.ascontiguousarray(p[0], dtype=_I32), np.ascontiguousarray(p[1], dtype=_I32),
            np.ascontiguousarray(v, dtype=np.float64))
    return arrs, _csr_struct(arrs)


def run_hook(lib, op, pa, va, pb, vb, nrows, ncols, cap):
    """one call of GeneoTestSparseProduct with room for `cap` entries: (rowptr, col, val), or None beyond the capacity"""
    keep_a, sa = _struct(pa, va)
    pbs = None
    if pb is not None:
        keep_b, sb = _struct(pb, vb)
        pbs = C.byref(sb)
    rp = np.full(nrows + 1, -7, dtype=_I32)
    col = np.full(max(1, cap), -7, dtype=_I32)
    val = np.full(max(1, cap), np.nan)
    nnz = lib.GeneoTestSparseProduct(op, C.byref(sa), pbs, ncols, rp.ctypes.data_as(L.c_int_p), col.ctypes.data_as(L.c_int_p),
                                     val.ctypes.data_as(L.c_dbl_p), cap)
    assert nnz != -2, lib.PCGenEOGetError(None).decode()
    if nnz == -1:
        return None
    assert nnz == cap, "%d entries in the result, %d in the reference" % (nnz, cap)
    return rp, col[:nnz], val[:nnz]


class variant:
    """a validation switch of the HIP backend, restored on exit (the host twin has none)"""

    def __init__(self, lib, name, value, restore):
        self.lib, self.name, self.value, self.restore = lib, name, value, restore

    def __enter__(self):
        rc = self.lib.GeneoSetKernelVariant(self.name, self.value)
        assert rc == 0 or not is_hip(self.lib), "unknown switch %r" % self.name

    def __exit__(self, *a):
        self.lib.GeneoSetKernelVariant(self.name, self.restore)


def same(x, y):
    return all(u.shape == v.shape for u, v in zip(x, y)) and bool((x[0] == y[0]).all() and (x[1] == y[1]).all()) and \
        bool((x[2].view(np.uint64) == y[2].view(np.uint64)).all())


def note(what, **kw):
    print("[sparse-product] %s: %s" % (what, ", ".join("%s %s" % (k, v) for k, v in kw.items())))


def check_spgemm(lib, what, pa, pb, seed, report=None, overflow=False, draw=None):
    """all checks of the module's docstring on A B.  report: (group, deferred, scan depth) expected on the HIP backend.
    overflow: a row is beyond the capacities -- None on the HIP backend, in every form.  draw(kind): the values of A and
    B instead of random ones.  Returns the default results {"int": (rowptr, col, val), "real": ...} (empty where the
    product is None)."""
    hip = is_hip(lib)
    n, ncols = len(pa[0]) - 1, pb[2]
    assert pa[2] == len(pb[0]) - 1
    ref = Reference(pa, pb)
    rng = np.random.default_rng(seed)
    results = {}
    for kind in ("int", "real"):
        va, vb = draw(kind) if draw else (values(len(pa[1]), kind, rng), values(len(pb[1]), kind, rng))
        run = lambda: run_hook(lib, 0, pa, va, pb, vb, n, ncols, ref.nnz)
        got = run()
        rep = sparse_product_report(lib)
        rep = (rep["group"], rep["deferred"], rep["scan_depth"])
        if hip:
            if kind == "int":
                note(what, classes=class_counts(classify(pa, pb, pick_group(pa, pb))[0]), report=rep)
            assert report is None or rep == tuple(report), "%s: report %r, the host computed %r" % (what, rep, tuple(report))
        else:
            assert rep == (0, 0, 0), "%s: the host twin reports zeros, got %r" % (what, rep)
        forms = [("again", None), ("spgemm_fill_scan", (b"spgemm_fill_scan", 1, 0)), ("spgemm_small_rows", (b"spgemm_small_rows", 0, 1))]
        if overflow and hip:
            assert got is None, "%s: a row beyond the capacity must give None" % what
            for name, sw in forms[1:]:
                with variant(lib, *sw):
                    assert run() is None, "%s: a row beyond the capacity must give None under %s" % (what, name)
            continue
        assert got is not None, "%s: None although every row fits" % what
        rp, col, val = got
        assert (rp == ref.indptr).all(), "%s (%s data): indptr" % (what, kind)
        assert (col == ref.indices).all(), "%s (%s data): indices" % (what, kind)
        assert strictly_increasing(rp, col), "%s: columns not strictly increasing" % what
        if kind == "int":
            exact = ref.exact(pa, va, pb, vb)
            bad = np.flatnonzero(val.view(np.uint64) != exact.view(np.uint64))
            assert len(bad) == 0, "%s: %d entries differ from the exact product, first at %d: %r, exact %r" % (
                what, len(bad), bad[0], val[bad[0]], exact[bad[0]])
        else:
            s, sabs = ref.longdouble(va, vb)
            err = np.abs(val.astype(LD) - s)
            bound = (ref.count + 2) * LD(U) * sabs
            bad = np.flatnonzero(~(err <= bound))
            assert len(bad) == 0, "%s: %d entries beyond (t + 2) u |A||B|, first at %d: err %.3e bound %.3e" % (
                what, len(bad), bad[0], float(err[bad[0]]), float(bound[bad[0]]))
        for name, sw in forms:
            if sw is None:
                other = run()
            else:
                with variant(lib, *sw):
                    other = run()
            assert other is not None and same(got, other), "%s (%s data): %s gives other bits" % (what, kind, name)
        results[kind] = got
    return results


def check_transpose(lib, what, pa, seed, depth, overflow=False):
    """A^T: indptr, indices and the bits of data equal scipy's, columns strictly increasing, two runs agree, report"""
    hip = is_hip(lib)
    n, ncols = len(pa[0]) - 1, pa[2]
    va = values(len(pa[1]), "real", np.random.default_rng(seed))
    t = sp.csr_matrix((va, pa[1], pa[0]), shape=(n, ncols)).T.tocsr()
    t.sort_indices()
    assert t.nnz == len(va)
    res = []
    for rep_no in range(2):
        got = run_hook(lib, 1, pa, va, None, None, ncols, ncols, t.nnz)
        rep = sparse_product_report(lib)
        rep = (rep["group"], rep["deferred"], rep["scan_depth"])
        if hip:
            if rep_no == 0:
                note(what, report=rep)
            assert rep == (0, 0, depth), "%s: report %r, expected scan depth %d" % (what, rep, depth)
        else:
            assert rep == (0, 0, 0)
        if overflow and hip:
            assert got is None, "%s: a transposed row beyond TR_MAXROW must give None" % what
            continue
        assert got is not None, "%s: None although every row fits" % what
        rp, col, val = got
        assert (rp == t.indptr).all(), "%s: indptr" % what
        assert (col == t.indices).all(), "%s: indices" % what
        assert strictly_increasing(rp, col), "%s: columns not strictly increasing" % what
        assert (val.view(np.uint64) == t.data.view(np.uint64)).all(), "%s: data" % what
        res.append(got)
    assert len(res) < 2 or same(res[0], res[1]), "%s: not reproducible" % what


# ---------------------------------------------------------------------------------------------- the group pass
NB_G, NCOLS_G = 4096, 5000
B_EMPTY = (0, 2048, 4095)                       # empty rows of B in first, middle and last position of a row of A
B_RUN = np.arange(1, 321)                       # one entry each, columns 7, 8, 9 in turn
B_PAIR = np.arange(330, 340)                    # two entries each
B_DISTINCT = np.arange(400, 1401)               # one entry each, pairwise different columns
B_WIDE = np.arange(1500, 1520)                  # 64 entries each inside a window of 200 columns
FILL_NA = {8: (2, 6), 16: (7, 10), 32: (15, 19), 64: (31, 37)}      # entries of an ordinary row, by group width


def group_b(rng):
    rows = []
    for j in range(NB_G):
        if j in B_EMPTY:
            rows.append([])
        elif 1 <= j <= 320:
            rows.append([7 + j % 3])
        elif 330 <= j < 340:
            c = int(rng.integers(0, NCOLS_G - 10))
            rows.append([c, c + int(rng.integers(1, 10))])
        elif 400 <= j <= 1400:
            rows.append([1000 + j])
        elif 1500 <= j < 1520:
            rows.append(3000 + np.sort(rng.choice(200, size=64, replace=False)))
        else:
            rows.append(np.unique(rng.integers(0, NCOLS_G, size=rng.choice([1, 2, 3], p=[0.8, 0.15, 0.05]))))
    return pattern(rows, NCOLS_G)


def group_rows(G, rng, blen):
    """the rows of A every group case holds: name -> sorted rows of B"""
    k7 = min(G, 7) - 3
    lo = rng.choice(B_DISTINCT[B_DISTINCT < 2048], size=(k7 + 1) // 2, replace=False)
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "G products, all columns distinct": np.sort(rng.choice(B_DISTINCT, size=G, replace=False)),
        "G products on one column": np.sort(rng.choice(B_RUN[B_RUN % 3 == 1], size=G, replace=False)),
        "half on one column": np.sort(np.concatenate([rng.choice(B_RUN[B_RUN % 3 == 1], size=G // 2, replace=False),
                                                      rng.choice(B_DISTINCT, size=G // 2, replace=False)])),
        "empty rows of B first, middle, last": np.sort(np.concatenate([B_EMPTY, lo, 2100 + np.arange(k7 // 2)])),
        "empty rows of B only": np.asarray(B_EMPTY),
    }


def deferred_rows(G, rng):
    """rows the group pass must leave to the wave-per-row kernels: name -> (sorted rows of B, class)"""
    k = constants()
    d = lambda m: rng.choice(B_DISTINCT, size=m, replace=False)
    small = lambda t: SMALL64 if t <= k.SMALL_MAX else PREFIX
    return {
        "G + 1 products, na = G": (np.sort(np.concatenate([d(G - 1), B_PAIR[:1]])), small(G + 1)),
        "na = G + 1": (np.sort(d(G + 1)), small(G + 1)),
        "65 products": (np.sort(np.concatenate([B_WIDE[:1], d(1)])), PREFIX),
        "257 products": (np.sort(np.concatenate([B_WIDE[:4], d(1)])), PREFIX),
        "1025 products": (np.sort(np.concatenate([B_WIDE[:16], d(1)])), PREFIX),
        "na = 256": (B_RUN[:k.SPG_KMAX], PREFIX),
        "na = 257": (B_RUN[:k.SPG_KMAX + 1], SERIAL),
    }


def group_problem(G, n, seed, plant=False):
    """n rows around the average row of band G; every row fits its group unless `plant`: then the rows of `deferred_rows`
    stand alone among fitting rows and side by side, and one of them is the first row and one the last (which ones
    turns with G: over the four widths every kind stands at an end).  Returns the patterns, the rows by name and the
    planted rows {row: class}"""
    rng = np.random.default_rng(seed)
    pb = group_b(rng)
    blen = np.diff(pb[0])
    pool = np.setdiff1d(np.arange(NB_G), np.concatenate([B_WIDE, B_RUN]))
    rows, names = [], {}
    for i in range(n):
        while True:
            r = np.unique(pool[rng.integers(0, len(pool), size=rng.integers(FILL_NA[G][0], FILL_NA[G][1] + 1))])
            if blen[r].sum() <= G:
                break
        rows.append(r)
    special = group_rows(G, rng, blen)
    at = list(range(len(special))) + [n - 1 - i for i in range(len(special))] + [40 + 23 * i for i in range(len(special))]
    for j, i in enumerate(at):                            # first rows, last rows (the last row empty), and scattered
        name = list(special)[j % len(special)]
        rows[i] = special[name]
        names.setdefault(name, []).append(i)
    planted = {}
    if plant:
        dr = deferred_rows(G, rng)
        m = len(dr)
        at = [0] + [n - 1] + [300 + 61 * i for i in range(m)] + list(range(2000, 2000 + m))
        turn = (8, 16, 32, 64).index(G)
        kinds = [list(dr)[turn], list(dr)[-1 - turn]] + list(dr) + list(dr)
        for i, name in zip(at, kinds):                    # first row, last row, alone among fitting rows, side by side
            rows[i] = dr[name][0]
            planted[i] = dr[name][1]
            names.setdefault(name, []).append(i)
    return pattern(rows, NB_G), pb, names, planted


def _group_case(G):
    def case(lib):
        k = constants()
        n = 1027                                          # no multiple of the 4 * 64 / G rows of a workgroup: dead lanes
        assert n % (4 * 64 // G) != 0
        pa, pb, names, _ = group_problem(G, n, 200 + G)
        assert pick_group(pa, pb) == G
        cls, na, total = classify(pa, pb, G)
        assert (cls == GROUPED).all(), class_counts(cls)
        for name in ("G products, all columns distinct", "G products on one column"):
            assert all(na[i] == G and total[i] == G for i in names[name]) and len(names[name]) == 3
        assert all(na[i] == 0 for i in names["empty"]) and all(total[i] == 0 and na[i] == 3 for i in names["empty rows of B only"])
        for i in names["empty rows of B first, middle, last"]:
            r = pa[1][pa[0][i]:pa[0][i + 1]]
            assert r[0] == B_EMPTY[0] and r[-1] == B_EMPTY[2] and B_EMPTY[1] in r[1:-1] and total[i] > 0
        c = check_spgemm(lib, "group %d, %d rows" % (G, n), pa, pb, 300 + G, report=(G, 0, 0))["int"]
        for i in names["G products on one column"]:
            assert c[0][i + 1] - c[0][i] == 1               # one run of full length
        for i in names["G products, all columns distinct"]:
            assert c[0][i + 1] - c[0][i] == G
    case.__name__ = "case_spgemm_group_%d" % G
    return case


case_spgemm_group_8, case_spgemm_group_16, case_spgemm_group_32, case_spgemm_group_64 = [_group_case(g) for g in (8, 16, 32, 64)]


def case_spgemm_deferral(lib):
    """the generator of the group cases at 4100 rows (device scan), with rows the group pass cannot hold planted at the
    first row, the last row, alone among fitting rows and side by side"""
    n = 4100
    for G in (8, 16, 32, 64):
        pa, pb, names, planted = group_problem(G, n, 400 + G, plant=True)
        assert pick_group(pa, pb) == G
        cls, na, total = classify(pa, pb, G)
        assert 0 in planted and n - 1 in planted and len(planted) == 16
        for i, c in planted.items():
            assert cls[i] == c, (G, i, CLASS_NAMES[cls[i]], CLASS_NAMES[c])
        deferred = int((cls != GROUPED).sum())
        assert deferred == len(planted)
        assert {int(total[i]) for i in planted} >= {G + 1, 65, 257, 1025, 256} and {int(na[i]) for i in planted} >= {G, G + 1, 256, 257}
        check_spgemm(lib, "deferral, group %d, %d rows" % (G, n), pa, pb, 500 + G, report=(G, deferred, scan_depth(n)))


def case_spgemm_group_min_rows(lib):
    """a.n = 255 takes no group pass, a.n = 256 with the same rows does; the common rows have equal bits"""
    k = constants()
    for G in (8, 16, 32, 64):
        pa, pb, _, _ = group_problem(G, k.GROUP_MIN_ROWS, 600 + G)
        short = (pa[0][:k.GROUP_MIN_ROWS], pa[1][:pa[0][k.GROUP_MIN_ROWS - 1]], pa[2])
        assert pick_group(pa, pb) == G and pick_group(short, pb) == 0
        assert (classify(pa, pb, G)[0] == GROUPED).all() and (classify(short, pb, 0)[0] != GROUPED).all()
        rng = np.random.default_rng(700 + G)
        vals = {kind: (values(len(pa[1]), kind, rng), values(len(pb[1]), kind, rng)) for kind in ("int", "real")}
        full = check_spgemm(lib, "%d rows, group %d" % (k.GROUP_MIN_ROWS, G), pa, pb, 0, report=(G, 0, 0), draw=lambda kind: vals[kind])
        part = check_spgemm(lib, "%d rows, no group" % (k.GROUP_MIN_ROWS - 1), short, pb, 0, report=(0, 0, 0),
                            draw=lambda kind: (vals[kind][0][:len(short[1])], vals[kind][1]))
        for kind in ("int", "real"):
            f, p = full[kind], part[kind]
            m = p[0][-1]
            assert (f[0][:k.GROUP_MIN_ROWS] == p[0]).all() and (f[1][:m] == p[1]).all() and \
                (f[2][:m].view(np.uint64) == p[2].view(np.uint64)).all(), "common rows differ between the two paths (%s data)" % kind


# ---------------------------------------------------------------------------------------------- the wave-per-row kernels
def padded(rows_b, empties, na):
    """the row of A over rows_b, filled up to na entries with empty rows of B"""
    return np.sort(np.concatenate([rows_b, empties[:na - len(rows_b)]])).astype(np.int64)


def case_spgemm_numeric_rounds(lib):
    """product counts at the 64-lane batch (shuffle sort against hash) and at the 256-product round of the numeric pass,
    from rows of B of 1, 63, 64, 65, 255 and 256 entries (a segment then crosses a batch and a round), each count
    through the prefix table (na small and na = 256) and through the serial walk (na = 257 and more).  All columns lie
    in a window of 256, so every row fits; a row of B of 257 entries cannot be part of a fitting row (it is in
    case_spgemm_capacity)."""
    k = constants()
    rng = np.random.default_rng(801)
    lens = [1, 63, 64, 65, 255, 256]
    nb = 1 + 10 * len(lens) + 300
    blen = np.zeros(nb, dtype=np.int64)
    blen[1:61] = np.tile(lens, 10)                         # ten rows of every length, in turn; every other row is empty
    empties = np.flatnonzero(blen == 0)                    # row 0 and rows 61 ..: in front of and behind every segment
    empties = np.concatenate([empties[:1], empties[-1:], empties[1:-1]])
    pb = pattern([np.sort(rng.choice(k.SPG_MAXD, size=m, replace=False)) for m in blen], 300)
    recipes = {64: [[64], [1, 63]], 65: [[65], [1, 64], [64, 1]], 255: [[255], [63, 64, 64, 64]], 256: [[256], [1, 255]],
               257: [[1, 256], [1, 255, 1], [65, 64, 64, 64]], 1023: [[256, 256, 256, 255], [255, 256, 256, 256]],
               1024: [[256] * 4, [255, 1, 256, 256, 256]], 1025: [[1, 256, 256, 256, 256], [256, 256, 256, 256, 1],
                                                                  [65, 64, 256, 256, 255, 64, 65]]}
    rows, want = [], []
    for count, rs in recipes.items():
        for r in rs:
            pick, j = [], 0
            for m in r:                                     # the next row of B of that length: the segments keep their order
                j = next(i for i in range(j + 1, 61) if blen[i] == m)
                pick.append(j)
            assert blen[pick].sum() == count
            for na in (len(pick), k.SPG_KMAX, k.SPG_KMAX + 1, len(pick) + len(empties)):
                rows.append(padded(np.array(pick), empties, na))
                want.append(SERIAL if na > k.SPG_KMAX else (SMALL64 if count <= k.SMALL_MAX else PREFIX))
    pa = pattern(rows, nb)
    cls, na, total = classify(pa, pb, 0)
    assert pick_group(pa, pb) == 0 and (cls == np.array(want)).all()
    assert set(total) == set(recipes) and {k.SPG_KMAX, k.SPG_KMAX + 1} <= set(na)
    check_spgemm(lib, "numeric rounds", pa, pb, 802, report=(0, 0, 0))


def capacity_b(rng):
    """rows 1..6: 100 columns each, pairwise disjoint; 11..16 the same columns again; 20 + r (r = 12, 13, 55, 56, 57): r
    further columns; 80 + r: the same again; 150: 257 columns; 200..499 empty; 500..: one entry each"""
    rows = [[] for _ in range(1200)]
    for i in range(1, 7):
        rows[i] = rows[10 + i] = 100 * i + np.arange(100)
    for r in (12, 13, 55, 56, 57):
        rows[20 + r] = rows[80 + r] = 700 + np.arange(r)
    rows[150] = 1000 + np.arange(257)
    for j in range(500, 1200):
        rows[j] = [int(rng.integers(0, 4000))]
    return pattern(rows, 4000)


def capacity_row(d, twice):
    q, r = divmod(d, 100)
    rows_b = list(range(1, q + 1)) + ([20 + r] if r else [])
    if twice:
        rows_b += list(range(11, q + 11)) + ([80 + r] if r else [])
    return np.array(sorted(rows_b))


def case_spgemm_capacity(lib):
    """255 and 256 distinct columns in a row give a result; 257 give None; 512 give None by the count of the filled
    slots; 513 and 600 by probe exhaustion (the table holds SPG_HS keys): through the prefix table and the serial walk,
    always one such row among fitting ones.  Last, the same through a group pass that defers the row."""
    k = constants()
    rng = np.random.default_rng(811)
    pb = capacity_b(rng)
    empties = np.arange(200, 500)
    fill = lambda m: [np.sort(rng.choice(np.arange(500, 1200), size=rng.integers(0, 6), replace=False)) for _ in range(m)]
    for d in (k.SPG_MAXD - 1, k.SPG_MAXD):
        r = capacity_row(d, True)
        pa = pattern(fill(5) + [r, padded(r, empties, k.SPG_KMAX), padded(r, empties, k.SPG_KMAX + 1)] + fill(4), 1200)
        cls, na, total = classify(pa, pb, 0)
        assert class_counts(cls) == dict(grouped=0, small64=9, prefix=2, serial=1) and (total[5:8] == 2 * d).all()
        c = check_spgemm(lib, "%d distinct columns" % d, pa, pb, 812 + d, report=(0, 0, 0))["int"]
        assert (np.diff(c[0])[5:8] == d).all()
    assert k.SPG_HS == 2 * k.SPG_MAXD
    for d in (k.SPG_MAXD + 1, k.SPG_HS, k.SPG_HS + 1, 600):
        r = capacity_row(d, False)
        for na, want in ((len(r), PREFIX), (k.SPG_KMAX + 1, SERIAL)):
            pa = pattern(fill(5) + [padded(r, empties, na)] + fill(4), 1200)
            cls, _, total = classify(pa, pb, 0)
            assert cls[5] == want and total[5] == d and (cls[np.arange(10) != 5] == SMALL64).all()
            check_spgemm(lib, "%d distinct columns, %s" % (d, CLASS_NAMES[want]), pa, pb, 813 + d, report=(0, 0, 0), overflow=True)
    pa = pattern(fill(3) + [np.array([150])] + fill(3), 1200)        # one row of B of 257 entries
    assert classify(pa, pb, 0)[2][3] == k.SPG_MAXD + 1
    check_spgemm(lib, "a row of B of 257 entries", pa, pb, 814, report=(0, 0, 0), overflow=True)
    rows = fill(300)
    rows[170] = capacity_row(600, False)
    pa = pattern(rows, 1200)
    cls, _, _ = classify(pa, pb, 8)
    assert pick_group(pa, pb) == 8 and int((cls != GROUPED).sum()) == 1 and cls[170] == PREFIX
    check_spgemm(lib, "600 distinct columns in a deferred row", pa, pb, 815, report=(8, 1, 0), overflow=True)


def home_slot(col):
    k = constants()
    return ((np.asarray(col, dtype=np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) & np.uint64(k.SPG_HS - 1)


def case_spgemm_hash(lib):
    """the hash table under stress: a row whose 256 columns all have home slot 0 (multiples of 512), and a row whose 120
    columns have home slots of 480 and above, so that the probe chains wrap past slot 511; about 2000 products each
    (every column is hit from many lanes at once), column indices up to 3 000 000; through the prefix table and the
    serial walk"""
    k = constants()
    rng = np.random.default_rng(821)
    ncols = 3000001
    zero = np.sort(np.concatenate([rng.choice(np.arange(0, 5859), size=k.SPG_MAXD - 1, replace=False), [5859]])) * k.SPG_HS
    assert len(zero) == k.SPG_MAXD and (home_slot(zero) == 0).all() and zero.max() > 2999000
    cand = rng.choice(ncols, size=20000, replace=False)
    high = np.sort(cand[home_slot(cand) >= 480][:120])
    assert len(high) == 120 and (home_slot(high) >= k.SPG_HS - 32).all() and len(high) > 32     # 120 keys on 32 slots: they wrap
    rows = [[] for _ in range(400)]
    for j in range(0, 9):                                   # seven of eight columns each: new columns turn up in every row of B
        rows[j] = np.sort(rng.choice(zero, size=224, replace=False))
    for j in range(10, 29):
        rows[j] = np.sort(rng.choice(high, size=105, replace=False))
    assert len(np.unique(np.concatenate(rows[0:9]))) == 256 and len(np.unique(np.concatenate(rows[10:29]))) == 120
    pb = pattern(rows, ncols)
    empties = np.arange(100, 400)
    a, b = np.arange(0, 9), np.arange(10, 29)
    pa = pattern([a, b, padded(a, empties, k.SPG_KMAX + 1), padded(b, empties, k.SPG_KMAX + 1), [], a, b], 400)
    cls, na, total = classify(pa, pb, 0)
    assert list(cls) == [PREFIX, PREFIX, SERIAL, SERIAL, SMALL64, PREFIX, PREFIX] and total[0] == 2016 and total[1] == 1995
    c = check_spgemm(lib, "hash", pa, pb, 822, report=(0, 0, 0))["int"]
    assert list(np.diff(c[0])) == [256, 120, 256, 120, 0, 256, 120]


# ---------------------------------------------------------------------------------------------- the row-pointer scan
def scan_problem(n, seed):
    """prolongator-like A (0 .. 3 entries per row, a few heavier rows) times a small B with one entry per row"""
    rng = np.random.default_rng(seed)
    nb = 1000
    pb = (np.arange(nb + 1, dtype=_I32), rng.integers(0, 700, size=nb).astype(_I32), 700)
    cnt = rng.integers(0, 4, size=n)
    cnt[n - 3] = 0
    heavy = np.unique(np.concatenate([[0, 1, n // 2, n - 1], rng.integers(0, n, size=6)]))
    cnt[heavy] = rng.integers(9, 41, size=len(heavy))
    rp = np.concatenate([[0], np.cumsum(cnt)])
    row = np.repeat(np.arange(n), cnt)
    col = rng.integers(0, 500, size=n)[row] + (np.arange(rp[-1]) - rp[row]) * rng.integers(1, 11, size=n)[row]
    pa = (rp.astype(_I32), col.astype(_I32), nb)
    check_pattern(*pa)
    return pa, pb, len(heavy)


def check_scan(lib, n, seed):
    pa, pb, heavy = scan_problem(n, seed)
    cls, _, _ = classify(pa, pb, 8)
    assert pick_group(pa, pb) == 8 and int((cls != GROUPED).sum()) == heavy and (cls[cls != GROUPED] == SMALL64).all()
    check_spgemm(lib, "scan, %d rows" % n, pa, pb, seed + 1, report=(8, heavy, scan_depth(n)))


def case_spgemm_scan_edges(lib):
    """a.n = 4095, 4096, 4097: the host loop, then one level of block totals"""
    k = constants()
    assert [scan_depth(k.SCAN_MIN + d) for d in (-1, 0, 1)] == [0, 1, 1]
    for d in (-1, 0, 1):
        check_scan(lib, k.SCAN_MIN + d, 830 + d)


def case_spgemm_scan_1048576(lib):
    """1024 full blocks: their totals are scanned by one block"""
    k = constants()
    assert scan_depth(k.SCAN_B * k.SCAN_B) == 1
    check_scan(lib, k.SCAN_B * k.SCAN_B, 840)


def case_spgemm_scan_1048577(lib):
    """1025 blocks: the totals are themselves scanned in two blocks and added back"""
    k = constants()
    assert scan_depth(k.SCAN_B * k.SCAN_B + 1) == 2
    check_scan(lib, k.SCAN_B * k.SCAN_B + 1, 850)


# ---------------------------------------------------------------------------------------------- transpose
def columns_with_counts(counts, nrows, rng):
    """pattern with counts[c] entries in column c, in random rows"""
    rows = np.concatenate([rng.choice(nrows, size=m, replace=False) for m in counts] + [np.zeros(0, dtype=np.int64)])
    cols = np.repeat(np.arange(len(counts)), counts)
    a = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(nrows, len(counts)))
    a.sort_indices()
    assert a.nnz == sum(counts)
    return a.indptr.astype(_I32), a.indices.astype(_I32), len(counts)


def case_transpose_sort_sizes(lib):
    """column counts at every size of the bitonic sort of the transposed rows, and one beyond TR_MAXROW"""
    k = constants()
    rng = np.random.default_rng(861)
    counts = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024]
    assert max(counts) == k.TR_MAXROW
    order = rng.permutation(len(counts))
    counts = [counts[i] for i in order]
    check_transpose(lib, "transpose, sort sizes", columns_with_counts(counts, 1100, rng), 862, 0)
    counts.insert(5, k.TR_MAXROW + 1)
    check_transpose(lib, "transpose, a column of 1025", columns_with_counts(counts, 1100, rng), 863, 0, overflow=True)


def transpose_problems(ncols, seed):
    """a short-and-wide source (3 rows) and a tall one, both with trailing empty columns"""
    rng = np.random.default_rng(seed)
    used = ncols - 17
    wide = pattern([np.flatnonzero(rng.random(used) < 0.4) for _ in range(3)], ncols)
    n = ncols + 1000
    cnt = (rng.random(n) < 0.8).astype(np.int64)
    tall = (np.concatenate([[0], np.cumsum(cnt)]).astype(_I32), rng.integers(0, used, size=int(cnt.sum())).astype(_I32), ncols)
    return wide, tall


def check_transpose_scan(lib, ncols, seed):
    wide, tall = transpose_problems(ncols, seed)
    check_transpose(lib, "transpose, 3 x %d" % ncols, wide, seed + 1, scan_depth(ncols))
    check_transpose(lib, "transpose, %d x %d" % (len(tall[0]) - 1, ncols), tall, seed + 2, scan_depth(ncols))


def case_transpose_scan_edges(lib):
    k = constants()
    for d in (-1, 0, 1):
        check_transpose_scan(lib, k.SCAN_MIN + d, 870 + 3 * d)


def case_transpose_scan_1048576(lib):
    k = constants()
    check_transpose_scan(lib, k.SCAN_B * k.SCAN_B, 880)


def case_transpose_scan_1048577(lib):
    k = constants()
    check_transpose_scan(lib, k.SCAN_B * k.SCAN_B + 1, 890)


def case_sparse_products_of_empty_rows(lib):
    """matrices of empty rows: indptr is all zero (host loop and device scan), for the transpose and the product"""
    k = constants()
    for n, ncols in ((37, 50), (50, k.SCAN_MIN + 5)):
        check_transpose(lib, "transpose of %d empty rows, %d columns" % (n, ncols), pattern([[]] * n, ncols), 895, scan_depth(ncols))
    pb = pattern([[1], [], [0, 2]], 3)
    check_spgemm(lib, "product of 300 empty rows", pattern([[]] * 300, 3), pb, 896, report=(8, 0, 0))
    check_spgemm(lib, "product of 9 empty rows", pattern([[]] * 9, 3), pb, 897, report=(0, 0, 0))
    check_spgemm(lib, "product over empty rows of B only", pattern([[1]] * 9, 3), pb, 898, report=(0, 0, 0))


CASES = [case_spgemm_group_8, case_spgemm_group_16, case_spgemm_group_32, case_spgemm_group_64, case_spgemm_deferral,
         case_spgemm_group_min_rows, case_spgemm_numeric_rounds, case_spgemm_capacity, case_spgemm_hash,
         case_spgemm_scan_edges, case_spgemm_scan_1048576, case_spgemm_scan_1048577, case_transpose_sort_sizes,
         case_transpose_scan_edges, case_transpose_scan_1048576, case_transpose_scan_1048577,
         case_sparse_products_of_empty_rows]
SPGEMM_CASES = [f.__name__ for f in CASES if f.__name__.startswith("case_spgemm")] + ["case_sparse_products_of_empty_rows"]
TRANSPOSE_CASES = [f.__name__ for f in CASES if f.__name__.startswith("case_transpose")] + ["case_sparse_products_of_empty_rows"]
