"""Host-side mirror of the reference's PC-shell interface (hdr/geneo.hpp, hdr/geneo_c.h) on top of
the C ABI of libgeneopc.so.  Same call order as the reference driver (src/geneo4PETSc.cpp:1328-1367):

    pc = GenEOPC()                       # PCRegister("geneo", createGenEOPC) + PCSetType
    pc.set_from_options(argv)            # PCSetFromOptions        -> setUpGenEOPCFromOptions
    pc.init(...) | pc.add_subdomain(...) # initGenEOPC / PCGenEOSetup
    pc.setup(b)                          # KSPSetUp                -> setUpGenEOPC
    x, its, rnorm, reason = pc.solve(b)  # KSPSolve (x0 from the PC, guess flagged non zero)
    y = pc.apply(x)                      # ops->apply              -> applyGenEOPC
    pc.destroy()                         # PCDestroy               -> destroyGenEOPC

All numerics run in the HIP library; numpy arrays are only staging for inputs and results.
"""
import ctypes as C

import numpy as np

from . import _lib as L

KSP_REASONS = {2: "KSP_CONVERGED_RTOL", 3: "KSP_CONVERGED_ATOL", -3: "KSP_DIVERGED_ITS", -4: "KSP_DIVERGED_DTOL",
               -5: "KSP_DIVERGED_BREAKDOWN",
               -8: "KSP_DIVERGED_INDEFINITE_MAT", -9: "KSP_DIVERGED_NANORINF", 0: "KSP_CONVERGED_ITERATING"}


class GenEOError(RuntimeError):
    pass


def _csr_arrays(a):
    """scipy csr_matrix or (rowptr, col, val) -> contiguous int32/int32/float64 arrays."""
    if hasattr(a, "indptr"):
        a = a.tocsr()
        a.sort_indices()
        rp, col, val = a.indptr, a.indices, a.data
    else:
        rp, col, val = a
    return (np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32),
            np.ascontiguousarray(val, dtype=np.float64))


def _csr_struct(arrs):
    rp, col, val = arrs
    return L.GeneoCsr(len(rp) - 1, rp.ctypes.data_as(L.c_int_p), col.ctypes.data_as(L.c_int_p),
                      val.ctypes.data_as(L.c_dbl_p))


class DeviceVector:
    """FP64 vector in HBM, allocated by the library."""

    def __init__(self, lib, n):
        self.lib, self.n = lib, int(n)
        self.ptr = lib.GeneoDeviceAlloc(max(1, self.n) * 8)
        if not self.ptr:
            raise GenEOError("device allocation failed")

    @classmethod
    def from_host(cls, lib, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        v = cls(lib, a.size)
        if a.size and lib.GeneoH2D(v.ptr, a.ctypes.data, a.size * 8):
            raise GenEOError("H2D failed")
        return v

    def to_host(self):
        out = np.empty(self.n, dtype=np.float64)
        if self.n and self.lib.GeneoD2H(out.ctypes.data, self.ptr, self.n * 8):
            raise GenEOError("D2H failed")
        return out

    def free(self):
        if self.ptr:
            self.lib.GeneoDeviceFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GenEOPC:
    def __init__(self, lib=None):
        self.lib = lib if lib is not None else L.load()
        self.h = C.c_void_p()
        if self.lib.PCCreate_GenEO(C.byref(self.h)):
            raise GenEOError("createGenEOPC failed")
        self.n_owned = None
        self._keep = []

    # -- errors / names --------------------------------------------------------------------
    def _chk(self, rc):
        if rc:
            raise GenEOError(self.lib.PCGenEOGetError(self.h).decode())

    @property
    def name(self):
        return self.lib.PCGenEOGetName(self.h).decode()

    def options(self):
        """The parsed options (the public parameter fields of the reference's geneoContext)."""
        out = {}
        for kv in self.lib.PCGenEOGetOptionsString(self.h).decode().split(";"):
            k, _, v = kv.partition("=")
            if k in ("dls1_pc", "els2_pc", "ksp_type", "dls1_ksp_type", "ksp_matsolve_type", "ksp_pc_side",
                     "ksp_fcg_truncation_type", "ksp_norm_type"):
                out[k] = v
            elif k == "dls1_cheb_safety":
                out[k] = tuple(float(t) for t in v.split(","))
            elif "." in v or "e" in v or "inf" in v:
                out[k] = float(v)
            else:
                out[k] = int(v)
        return out

    def usage(self):
        return self.lib.usageGenEO_c().decode()

    # -- options -----------------------------------------------------------------------------
    def set_from_options(self, argv):
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        self._chk(self.lib.PCSetFromOptions_GenEO(self.h, len(argv), arr))

    def set_option(self, key, value=""):
        self._chk(self.lib.PCGenEOSetOption(self.h, key.encode(), str(value).encode()))

    # -- inputs ------------------------------------------------------------------------------
    def set_sizes(self, nb_dof, nb_sub_global):
        self.N = int(nb_dof)
        self._chk(self.lib.PCGenEOSetSizes(self.h, int(nb_dof), int(nb_sub_global)))
        if self.n_owned is None:
            self.n_owned = int(nb_dof)

    def add_subdomain(self, gid, l2g, mult, a_neu, a_dir=None):
        l2g = np.ascontiguousarray(l2g, dtype=np.int32)
        mult = np.ascontiguousarray(mult, dtype=np.int32)
        an = _csr_arrays(a_neu)
        sn = _csr_struct(an)
        sd = None
        if a_dir is not None:
            ad = _csr_arrays(a_dir)
            sd = _csr_struct(ad)
        self._chk(self.lib.PCGenEOAddSubdomain(self.h, int(gid), len(l2g), l2g.ctypes.data_as(L.c_int_p),
                                               mult.ctypes.data_as(L.c_int_p), C.byref(sn),
                                               C.byref(sd) if sd is not None else None))

    def setup_from_operators(self, nbDOF, pcMap, a_local, dofMultiplicities, pcADirLoc=None, dofIntersections=None):
        """The reference's PETSc-style pair (hdr/geneo_c.h:10): KSPSetOperators(MATIS A) then
        PCGenEOSetup(pc, pcADirLoc, dofMultiplicities, dofIntersections) -- one subdomain for this rank."""
        l2g = np.ascontiguousarray(pcMap, dtype=np.int32)
        mult = np.ascontiguousarray(dofMultiplicities, dtype=np.int32)
        an = _csr_arrays(a_local)
        mat = L.GeneoMatIS(int(nbDOF), len(l2g), l2g.ctypes.data_as(L.c_int_p), _csr_struct(an))
        self.N = int(nbDOF)
        if self.n_owned is None:
            self.n_owned = int(nbDOF)
        self._chk(self.lib.PCSetOperators_GenEO(self.h, C.byref(mat)))
        sd = None
        if pcADirLoc is not None:
            ad = _csr_arrays(pcADirLoc)
            sd = _csr_struct(ad)
        inter = None
        if dofIntersections is not None:
            keep = [np.ascontiguousarray(x, dtype=np.int32) for x in dofIntersections]
            inter = (L.GeneoIS * len(keep))(*[L.GeneoIS(len(x), x.ctypes.data_as(L.c_int_p)) for x in keep])
        self._chk(self.lib.PCGenEOSetup(self.h, C.byref(sd) if sd is not None else None,
                                        L.GeneoIS(len(mult), mult.ctypes.data_as(L.c_int_p)), inter))

    def init(self, nbDOF, nbDOFLoc, pcMap, pcA, pcADirLoc, pcB, pcX0, dofIdxDomLoc, dofIdxMultLoc,
             intersectLoc=None):
        """initGenEOPC (hdr/geneo.hpp:30-35): one subdomain for this rank.  pcB: DeviceVector or None."""
        del pcX0, dofIdxDomLoc   # x0 is produced by setup; the map carries the DOF ids
        l2g = np.ascontiguousarray(pcMap, dtype=np.int32)
        mult = np.ascontiguousarray(dofIdxMultLoc, dtype=np.uint32)
        an = _csr_arrays(pcA)
        sn = _csr_struct(an)
        sd = None
        if pcADirLoc is not None:
            ad = _csr_arrays(pcADirLoc)
            sd = _csr_struct(ad)
        self.N = int(nbDOF)
        if self.n_owned is None:
            self.n_owned = int(nbDOF)
        self._chk(self.lib.initGenEOPC_c(self.h, int(nbDOF), int(nbDOFLoc), l2g.ctypes.data_as(L.c_int_p),
                                         C.byref(sn), C.byref(sd) if sd is not None else None,
                                         pcB.ptr if pcB is not None else None, None,
                                         mult.ctypes.data_as(C.POINTER(C.c_uint))))
        if intersectLoc is not None:
            self.set_intersect(getattr(self, "rank", 0), [len(x) > 0 for x in intersectLoc])

    def set_comm(self, rank, size, owned_gid, halo_gid, recv_counts, send_counts, send_idx, exchange, allreduce,
                 send_ptr, recv_ptr, red_ptr, red_capacity):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        owned_gid, halo_gid = i32(owned_gid), i32(halo_gid)
        recv_counts, send_counts, send_idx = i32(recv_counts), i32(send_counts), i32(send_idx)
        self._cb = (L.EXCHANGE_FN(exchange), L.ALLREDUCE_FN(allreduce))   # keep alive
        self._keep += [owned_gid, halo_gid, recv_counts, send_counts, send_idx]
        p = lambda a: a.ctypes.data_as(L.c_int_p)
        self._chk(self.lib.PCGenEOSetComm(self.h, rank, size, len(owned_gid), p(owned_gid), len(halo_gid),
                                          p(halo_gid), p(recv_counts), p(send_counts), p(send_idx), self._cb[0],
                                          self._cb[1], None, send_ptr, recv_ptr, red_ptr, int(red_capacity)))
        self.n_owned = len(owned_gid)
        self.rank = int(rank)

    def set_comm_width(self, width):
        """The halo buffers hold `width` vectors per exchange (PCGenEOSetCommWidth): blocked assembly of E."""
        self._chk(self.lib.PCGenEOSetCommWidth(self.h, int(width)))

    # -- PC ops ------------------------------------------------------------------------------
    def setup(self, b=None):
        """KSPSetUp -> setUpGenEOPC.  b: DeviceVector / numpy (needed only for the E-hybrid initial guess)."""
        self._b = self._as_dev(b) if b is not None else None
        if self._b is not None:
            self._chk(self.lib.PCGenEOSetRHS(self.h, self._b.ptr))
        self._chk(self.lib.PCSetUp_GenEO(self.h))

    def _as_dev(self, a):
        if isinstance(a, DeviceVector):
            return a
        return DeviceVector.from_host(self.lib, a)

    def _unary(self, fn, x):
        xd = self._as_dev(x)
        yd = DeviceVector(self.lib, xd.n)
        self._chk(fn(self.h, xd.ptr, yd.ptr))
        return yd if isinstance(x, DeviceVector) else yd.to_host()

    def apply(self, x):
        return self._unary(self.lib.PCApply_GenEO, x)

    def apply_q(self, x):
        return self._unary(self.lib.PCGenEOApplyQ, x)

    def matmult(self, x):
        return self._unary(self.lib.MatMult_GenEO, x)

    def x0(self):
        v = DeviceVector(self.lib, self.n_owned)
        self._chk(self.lib.PCGenEOGetX0(self.h, v.ptr))
        return v

    def solve(self, b, x0=None):
        """KSPSolve with the initial guess the PC produced (geneo.cpp:1601-1607) unless x0 is given."""
        bd = self._as_dev(b)
        xd = self._as_dev(x0) if x0 is not None else self.x0()
        its, reason, rnorm = C.c_int(0), C.c_int(0), C.c_double(0.0)
        self._chk(self.lib.KSPSolve_GenEO(self.h, bd.ptr, xd.ptr, C.byref(its), C.byref(rnorm), C.byref(reason)))
        x = xd if isinstance(b, DeviceVector) else xd.to_host()
        return x, its.value, rnorm.value, KSP_REASONS.get(reason.value, str(reason.value))

    # -- blocks of right-hand sides (-geneo_block_width 16 | 32) ----------------------------------
    def _block(self, fn, X):
        """X: (n_owned, m) array.  Staged column-major with ld = n_owned; returns the (n_owned, m) result."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise GenEOError("a block of right-hand sides is a 2-d array (n_owned, m)")
        n, m = X.shape
        xd = DeviceVector.from_host(self.lib, np.asfortranarray(X).ravel(order="F"))
        yd = DeviceVector(self.lib, n * max(1, m))
        out = fn(xd, yd, n, m)
        Y = yd.to_host()[:n * m].reshape((n, m), order="F")
        return Y if out is None else (Y,) + out

    def mat_apply(self, X):
        """PCMatApply_GenEO: M^-1 on every column of X, in slabs of the block width."""
        return self._block(lambda xd, yd, n, m: self._chk(self.lib.PCMatApply_GenEO(self.h, xd.ptr, n, yd.ptr, n, m)), X)

    def mat_mult(self, X):
        """MatMatMult_GenEO: the MATIS operator on every column of X."""
        return self._block(lambda xd, yd, n, m: self._chk(self.lib.MatMatMult_GenEO(self.h, xd.ptr, n, yd.ptr, n, m)), X)

    def mat_solve(self, B):
        """KSPMatSolve_GenEO: block PCG (or, -ksp_matsolve_type gmres, block GMRES) from a zero initial guess.  Returns (X, its, rnorm, reasons) with one entry per
        column; reasons are the KSPConvergedReason names."""
        def run(bd, xd, n, m):
            its, rs, rn = np.zeros(max(1, m), dtype=np.int32), np.zeros(max(1, m), dtype=np.int32), np.zeros(max(1, m))
            self._chk(self.lib.KSPMatSolve_GenEO(self.h, bd.ptr, n, xd.ptr, n, m, its.ctypes.data_as(L.c_int_p),
                                                 rn.ctypes.data_as(L.c_dbl_p), rs.ctypes.data_as(L.c_int_p)))
            return its[:m], rn[:m], [KSP_REASONS.get(int(r), str(int(r))) for r in rs[:m]]
        return self._block(run, B)

    def block_info(self):
        """PCGenEOGetBlockInfo since the set-up: width, slabs and columns through the block apply, zero columns that padded
        them, local solves of slabs replayed from the HIP graph."""
        w = C.c_int(0)
        v = [C.c_longlong(0) for _ in range(4)]
        if self.lib.PCGenEOGetBlockInfo(self.h, C.byref(w), *[C.byref(x) for x in v]) < 0:
            raise GenEOError("PCGenEOGetBlockInfo: bad handle")
        return dict(width=w.value, slabs=v[0].value, columns=v[1].value, padded=v[2].value, graph_launches=v[3].value)

    def block_krylov_info(self):
        """PCGenEOGetBlockKrylovInfo: basis slabs and device bytes the block GMRES (-ksp_matsolve_type gmres) holds now, and
        since the set-up its Gram-Schmidt passes through the fused kernels and through their composed forms."""
        s, b = C.c_int(0), C.c_double(0.0)
        v = [C.c_longlong(0) for _ in range(2)]
        if self.lib.PCGenEOGetBlockKrylovInfo(self.h, C.byref(s), C.byref(b), *[C.byref(x) for x in v]) < 0:
            raise GenEOError("PCGenEOGetBlockKrylovInfo: bad handle")
        return dict(basis_slabs=s.value, basis_bytes=b.value, gs_fused=v[0].value, gs_composed=v[1].value)

    def krylov_info(self):
        """PCGenEOGetKrylovInfo: device vectors and bytes the right-preconditioned / flexible GMRES (-ksp_pc_side right,
        -ksp_type fgmres) holds now, since the set-up its Gram-Schmidt passes through the fused kernels and through their
        composed forms, and the preconditioner applications and operator products of the last solve()."""
        s, b = C.c_int(0), C.c_double(0.0)
        v = [C.c_longlong(0) for _ in range(4)]
        if self.lib.PCGenEOGetKrylovInfo(self.h, C.byref(s), C.byref(b), *[C.byref(x) for x in v]) < 0:
            raise GenEOError("PCGenEOGetKrylovInfo: bad handle")
        return dict(basis_vectors=s.value, basis_bytes=b.value, gs_fused=v[0].value, gs_composed=v[1].value,
                    pc_applies=v[2].value, mat_mults=v[3].value)

    def fcg_info(self):
        """PCGenEOGetFcgInfo: direction / product pairs and device bytes the flexible CG (-ksp_type fcg) holds now, since the
        set-up its steps through the fused kernel and through its composed form, and of the last fcg solve the largest
        window and the downloads the host waited for."""
        d, b, w = C.c_int(0), C.c_double(0.0), C.c_int(0)
        v = [C.c_longlong(0) for _ in range(3)]
        if self.lib.PCGenEOGetFcgInfo(self.h, C.byref(d), C.byref(b), C.byref(v[0]), C.byref(v[1]), C.byref(w), C.byref(v[2])) < 0:
            raise GenEOError("PCGenEOGetFcgInfo: bad handle")
        return dict(directions=d.value, bytes=b.value, steps_fused=v[0].value, steps_composed=v[1].value,
                    max_window=w.value, downloads=v[2].value)

    def coarse_block_counters(self):
        """PCGenEOGetCoarseBlockCounters since the set-up: slab applications of E^-1 by the blocked sweeps on the whole block,
        column by column through the single-vector path, and by one host round trip of the block."""
        v = [C.c_longlong(0) for _ in range(3)]
        if self.lib.PCGenEOGetCoarseBlockCounters(self.h, *[C.byref(x) for x in v]) < 0:
            raise GenEOError("PCGenEOGetCoarseBlockCounters: bad handle")
        return dict(blocked=v[0].value, by_column=v[1].value, host_blocks=v[2].value)

    def residual_history(self):
        n = self.lib.PCGenEOGetResidualHistory(self.h, None, 0)
        out = np.zeros(max(1, n))
        self.lib.PCGenEOGetResidualHistory(self.h, out.ctypes.data_as(L.c_dbl_p), n)
        return out[:n]

    # -- results -------------------------------------------------------------------------------
    def info(self):
        i = L.GeneoInfo()
        self._chk(self.lib.PCGenEOGetInfo(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in L.GeneoInfo._fields_}

    def eigenvalues(self, local_sub, candidates=False):
        fn = self.lib.PCGenEOGetCandidates if candidates else self.lib.PCGenEOGetEigenvalues
        n = fn(self.h, local_sub, None, 0)
        if n < 0:
            raise GenEOError("no such subdomain")
        out = np.zeros(max(1, n))
        fn(self.h, local_sub, out.ctypes.data_as(L.c_dbl_p), n)
        return out[:n]

    def E(self):
        d = self.lib.PCGenEOGetE(self.h, None, 0)
        out = np.zeros(max(1, d * d))
        self.lib.PCGenEOGetE(self.h, out.ctypes.data_as(L.c_dbl_p), d * d)
        return out[:d * d].reshape(d, d)

    def set_intersect(self, gid, nonempty):
        """intersectLoc emptiness flags of subdomain gid (initGenEOPC, hdr/geneo.hpp:34); GenEO-2 only."""
        f = np.ascontiguousarray(nonempty, dtype=np.int32)
        self._chk(self.lib.PCGenEOSetIntersect(self.h, int(gid), len(f), f.ctypes.data_as(L.c_int_p)))

    def local_params(self):
        """(tau_loc, gamma_loc) per local subdomain (getLocalGenEOTau / Gamma, geneo.cpp:1097-1232)."""
        n = self.lib.PCGenEOGetLocalParams(self.h, None, None, 0)
        t, g = np.zeros(max(1, n)), np.zeros(max(1, n))
        self.lib.PCGenEOGetLocalParams(self.h, t.ctypes.data_as(L.c_dbl_p), g.ctypes.data_as(L.c_dbl_p), n)
        return t[:n], g[:n]

    def coarse_info(self):
        """(dimE, factor_on_device, solve_kind, block) after the set-up (PCGenEOGetCoarseInfo): whether the blocked device
        factorisation made the factor of E, and how E^-1 is applied -- 0 host round trip, 1 one-workgroup device sweeps,
        2 blocked device sweeps with that block size."""
        v = [C.c_int(0) for _ in range(4)]
        self._chk(self.lib.PCGenEOGetCoarseInfo(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def local_solver_info(self):
        """Chebyshev local solver (-dls1_ksp_type chebyshev), after the set-up: per local subdomain the bounds lo, hi of the
        V-cycle-preconditioned operator, the degree k_s and the residual reduction of the set-up's verification solve
        (PCGenEOGetLocalSolverInfo).  Four empty arrays on the cg path."""
        n = self.lib.PCGenEOGetLocalSolverInfo(self.h, None, None, None, None, 0)
        if n < 0:
            raise GenEOError("PCGenEOGetLocalSolverInfo: bad handle")
        lo, hi, ach = np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros(max(1, n))
        its = np.zeros(max(1, n), dtype=np.int32)
        self.lib.PCGenEOGetLocalSolverInfo(self.h, lo.ctypes.data_as(L.c_dbl_p), hi.ctypes.data_as(L.c_dbl_p),
                                           its.ctypes.data_as(L.c_int_p), ach.ctypes.data_as(L.c_dbl_p), n)
        return lo[:n], hi[:n], its[:n], ach[:n]

    def local_solver_table(self):
        """The Chebyshev coefficient table of the device, shape (K, nsub, 2): (a_k, b_k) per step and local subdomain."""
        ns = self.lib.PCGenEOGetLocalSolverInfo(self.h, None, None, None, None, 0)
        K = self.lib.PCGenEOGetLocalSolverTable(self.h, None, 0)
        if K < 0 or ns < 0:
            raise GenEOError(self.lib.PCGenEOGetError(self.h).decode())
        t = np.zeros(max(1, K * ns * 2))
        self.lib.PCGenEOGetLocalSolverTable(self.h, t.ctypes.data_as(L.c_dbl_p), K * ns * 2)
        return t[:K * ns * 2].reshape(K, ns, 2)

    def local_solver_counters(self):
        """What the Chebyshev local solves ran since the last set-up (PCGenEOGetLocalSolverCounters): K steps per solve,
        solves in all, solves replayed from the HIP graph, residual updates taken by the fused sliced kernel."""
        v = [C.c_longlong(0) for _ in range(3)]
        K = self.lib.PCGenEOGetLocalSolverCounters(self.h, *[C.byref(x) for x in v])
        if K < 0:
            raise GenEOError("PCGenEOGetLocalSolverCounters: bad handle")
        return dict(K=K, solves=v[0].value, graph_launches=v[1].value, fused_residuals=v[2].value)

    def local_dims(self):
        n = self.lib.PCGenEOGetLocalDims(self.h, None, 0)
        out = np.zeros(max(1, n), dtype=np.int32)
        self.lib.PCGenEOGetLocalDims(self.h, out.ctypes.data_as(L.c_int_p), n)
        return out[:n]

    def destroy(self):
        if self.h:
            self.lib.PCDestroy_GenEO(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def sparse_product(a, b=None, lib=None):
    """Device sparse products of the multigrid set-up through the test hook: A @ B, or A.T when b is None.
    Returns a scipy csr_matrix, or None when a row exceeds the kernels' per-row capacity."""
    import scipy.sparse as sp
    lib = lib if lib is not None else L.load()
    aa = _csr_arrays(a)
    sa = _csr_struct(aa)
    op, ncols, sb = 1, a.shape[1], None
    if b is not None:
        ba = _csr_arrays(b)
        sb = _csr_struct(ba)
        op, ncols = 0, b.shape[1]
    nrows = a.shape[0] if b is not None else a.shape[1]
    pb = C.byref(sb) if sb is not None else None
    nnz = lib.GeneoTestSparseProduct(op, C.byref(sa), pb, ncols, None, None, None, 0)
    if nnz == -1:
        return None
    if nnz < 0:
        raise GenEOError(lib.PCGenEOGetError(None).decode())
    rp, col, val = np.zeros(nrows + 1, dtype=np.int32), np.zeros(max(1, nnz), dtype=np.int32), np.zeros(max(1, nnz))
    lib.GeneoTestSparseProduct(op, C.byref(sa), pb, ncols, rp.ctypes.data_as(L.c_int_p), col.ctypes.data_as(L.c_int_p),
                               val.ctypes.data_as(L.c_dbl_p), nnz)
    return sp.csr_matrix((val[:nnz], col[:nnz], rp), shape=(nrows, ncols if b is not None else a.shape[0]))


def sparse_product_report(lib=None):
    """What the calling thread's last sparse_product decided: the lanes per row of the short-row pass (`group`: 0, 8,
    16, 32, 64), the rows it left to the wave-per-row kernels (`deferred`) and the depth of the row-pointer scan
    (`scan_depth`: 0 host loop, 1 one level of block totals, 2 totals scanned in more than one block)."""
    lib = lib if lib is not None else L.load()
    g, d, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    lib.GeneoTestSparseProductReport(C.byref(g), C.byref(d), C.byref(s))
    return dict(group=g.value, deferred=d.value, scan_depth=s.value)


class Spmv:
    """Stand-alone CSR SpMV / SpMM handle (the roofline kernel of bench.py)."""

    def __init__(self, a, lib=None):
        self.lib = lib if lib is not None else L.load()
        arrs = _csr_arrays(a)
        self.n = len(arrs[0]) - 1
        self.nnz = int(arrs[0][-1])
        self.h = C.c_void_p()
        s = _csr_struct(arrs)
        if self.lib.GeneoSpmvCreate(C.byref(s), C.byref(self.h)):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())

    def apply(self, x):
        xd = x if isinstance(x, DeviceVector) else DeviceVector.from_host(self.lib, x)
        yd = DeviceVector(self.lib, self.n)
        if self.lib.GeneoSpmvApply(self.h, xd.ptr, yd.ptr):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())
        return yd if isinstance(x, DeviceVector) else yd.to_host()

    def time(self, xd, yd, reps):
        ms = C.c_double(0.0)
        if self.lib.GeneoSpmvTime(self.h, xd.ptr, yd.ptr, int(reps), C.byref(ms)):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())
        return ms.value

    def spmm(self, X, pre=None, post=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        n, m = X.shape
        xd = DeviceVector.from_host(self.lib, X.ravel())
        yd = DeviceVector(self.lib, self.n * m)
        pr = DeviceVector.from_host(self.lib, pre) if pre is not None else None
        po = DeviceVector.from_host(self.lib, post) if post is not None else None
        if self.lib.GeneoSpmmApply(self.h, xd.ptr, yd.ptr, m, pr.ptr if pr else None, po.ptr if po else None):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())
        return yd.to_host().reshape(self.n, m)

    def fused(self, epi, X=None, B=None, Z=None, dinv=None, w=0.0):
        """Multigrid epilogues fused into the SpMV / SpMM launch (GeneoSpmmFused); returns (Y, Z_out)."""
        ref = X if X is not None else B
        ref = np.asarray(ref, dtype=np.float64)
        m = 1 if ref.ndim == 1 else ref.shape[1]
        dev = lambda a: DeviceVector.from_host(self.lib, np.ascontiguousarray(a, dtype=np.float64).ravel()) if a is not None else None
        xd, bd, dd = dev(X), dev(B), dev(dinv)
        zd = dev(Z) if Z is not None else (DeviceVector(self.lib, self.n * m) if epi == 4 else None)
        yd = DeviceVector(self.lib, self.n * m)
        p = lambda v: v.ptr if v is not None else None
        if self.lib.GeneoSpmmFused(self.h, int(epi), p(xd), yd.ptr, m, p(bd), p(zd), p(dd), float(w)):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())
        shape = (self.n,) if ref.ndim == 1 else (self.n, m)
        return yd.to_host().reshape(shape), (zd.to_host().reshape(shape) if zd is not None else None)

    def fused_single(self, epi, X=None, B=None, Z=None, dinv=None, w=0.0):
        """The single-vector launches of `fused` (epi 0: A X) on the single-precision companion of the matrix."""
        dev = lambda a: DeviceVector.from_host(self.lib, np.ascontiguousarray(a, dtype=np.float64).ravel()) if a is not None else None
        xd, bd, dd = dev(X), dev(B), dev(dinv)
        zd = dev(Z) if Z is not None else (DeviceVector(self.lib, self.n) if epi == 4 else None)
        yd = DeviceVector(self.lib, self.n)
        p = lambda v: v.ptr if v is not None else None
        if self.lib.GeneoSpmvFusedSingle(self.h, int(epi), p(xd), yd.ptr, p(bd), p(zd), p(dd), float(w)):
            raise GenEOError(self.lib.PCGenEOGetError(None).decode())
        return yd.to_host(), (zd.to_host() if zd is not None else None)

    def offset_info(self):
        """(slices, coded slices) of the offset coding of the columns (made with the companion: after fused_single)."""
        ns, nc = C.c_int(0), C.c_int(0)
        if self.lib.GeneoSpmvOffsetInfo(self.h, C.byref(ns), C.byref(nc)):
            raise GenEOError("GeneoSpmvOffsetInfo failed")
        return ns.value, nc.value

    def algorithmic_bytes(self):
        """nnz*(8+4) + (n+1)*4 + n*8 (x once) + n*8 (y)."""
        return self.nnz * 12 + (self.n + 1) * 4 + self.n * 16

    def destroy(self):
        if self.h:
            self.lib.GeneoSpmvDestroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def block_kernel(kind, suboff, S, TC, lib=None, reps=0):
    """kind 0: per-subdomain Gram S^T T (kind 2: the same through the two-left-block entry) ; kind 1: per-subdomain
    S C.  Returns (result, ms_avg)."""
    lib = lib if lib is not None else L.load()
    suboff = np.ascontiguousarray(suboff, dtype=np.int32)
    nsub = len(suboff) - 1
    S = np.ascontiguousarray(S, dtype=np.float64)
    TC = np.ascontiguousarray(TC, dtype=np.float64)
    n, p = S.shape
    if kind in (0, 2):
        q = TC.shape[1]
        out = np.zeros((nsub, p, q))
    else:
        q = TC.shape[2]
        out = np.zeros((n, q))
    ms = C.c_double(0.0)
    rc = lib.GeneoBlockKernel(kind, nsub, suboff.ctypes.data_as(L.c_int_p), S.ctypes.data_as(L.c_dbl_p), p,
                              TC.ctypes.data_as(L.c_dbl_p), q, out.ctypes.data_as(L.c_dbl_p), int(reps),
                              C.byref(ms))
    if rc:
        raise GenEOError(lib.PCGenEOGetError(None).decode())
    return out, ms.value
