"""-m gpu: the Chebyshev local solver (-dls1_ksp_type chebyshev) on the device, through the C ABI: the step kernel alone
(cheb_dev.hip, GeneoTestPrimitive("cheb_dir")), the apply with both fused kernels (step and residual update) against the
apply with both composed forms, the GPU against the dense inverses and against the host twin, graph replay and re-set-up
with the counters of what ran, and the outer GMRES count.

cheb_dir evaluates d = fl(fl(a z) + fl(b d)), x = fl(x + d), out = fl(dscale x) with contraction off (DESIGN.md section
4.1): numpy's float64 expressions below are the same roundings, so the 2 ulp bar of the kernel test has room to spare."""
import ctypes as C

import numpy as np
import pytest

import cases
from primitive_cases import Buf, SENTF

pytestmark = pytest.mark.gpu

BASE = ["-geneo_tau", "0.2", "-geneo_cut", "4"]
CHEB = ["-dls1_ksp_type", "chebyshev"]


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()          # raises if the HIP library is missing: no fallback


@pytest.fixture(scope="module")
def host():
    from hostsim_util import hostsim_lib
    return hostsim_lib()


@pytest.fixture(scope="module")
def case20():
    return cases.grid_case(n=20, parts=(2, 2, 2), overlap=2)


@pytest.fixture(scope="module")
def case12():
    return cases.grid_case(n=12, parts=(2, 2, 2), overlap=2)


def argv_for(lvl, ksp="gmres", extra=()):
    return ["-geneo_lvl", lvl, "-ksp_type", ksp] + BASE + list(extra)


class fused_off:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.GeneoSetKernelVariant(b"cheb_fused", 0) == 0

    def __exit__(self, *a):
        assert self.lib.GeneoSetKernelVariant(b"cheb_fused", 1) == 0


# ---- 8. the kernel alone --------------------------------------------------------------------------------------------
SUBS = (1, 1025, 197)        # a one-row chunk; a chunk boundary with a one-row tail; no multiple of 64 or of the vector width


def ulp_diff(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64)).max() if a.size else 0


def run_cheb_dir(lib, flags, with_dscale, shift, zero_sub=2, seed=5):
    """shift = 1: every vector starts one double into its buffer (8-byte aligned only: the scalar form of the kernel)"""
    rng = np.random.default_rng(seed + 10 * flags + shift)
    off = np.concatenate([[0], np.cumsum(SUBS)]).astype(np.int32)
    n, ns = int(off[-1]), len(SUBS)
    coef = rng.random((ns, 2)) + 0.25
    coef[:, 1] *= -1.0 if flags & 1 else 1.0
    if zero_sub is not None:
        coef[zero_sub] = 0.0
    z, d, x, ds = (rng.standard_normal(n) for _ in range(4))
    lead = np.full(shift, SENTF)
    bufs = {k: Buf(lib, np.concatenate([lead, v])) for k, v in
            dict(coef=coef.reshape(-1), z=z, d=d, x=x, ds=ds, out=np.full(n, SENTF)).items()}
    ptr = lambda k: bufs[k].ptr + (8 * shift if k != "coef" else 0)
    ia = (C.c_int * 2)(ns, flags)
    da = (C.c_double * 1)(0.0)
    pa = (C.c_void_p * 7)(off.ctypes.data, bufs["coef"].ptr if not shift else bufs["coef"].ptr + 8, ptr("z"), ptr("d"), ptr("x"),
                          ptr("ds") if with_dscale else None, ptr("out"))
    rc = lib.GeneoTestPrimitive(b"cheb_dir", ia, da, pa)
    assert rc == 1, (rc, lib.PCGenEOGetError(None).decode())
    got = {k: bufs[k].get()[shift:] for k in bufs}          # .get() checks both canaries of every buffer
    for k in bufs:
        assert np.array_equal(bufs[k].get()[:shift], lead), "write in front of " + k
    a = np.repeat(coef[:, 0], SUBS)
    b = np.repeat(coef[:, 1], SUBS)
    if flags & 1:
        d_ref = a * z
        x_ref = d_ref.copy()
    else:
        d_ref = a * z + b * d
        x_ref = x + d_ref
    out_ref = (ds * x_ref if with_dscale else x_ref) if flags & 2 else np.full(n, SENTF)
    assert np.array_equal(got["z"], z) and np.array_equal(got["ds"], ds) and np.array_equal(got["coef"], coef.reshape(-1))
    for k, ref in (("d", d_ref), ("x", x_ref), ("out", out_ref)):
        assert ulp_diff(got[k], ref) <= 2, (k, flags, with_dscale, shift, ulp_diff(got[k], ref))
    if zero_sub is not None:
        r0, r1 = off[zero_sub], off[zero_sub + 1]
        assert np.all(got["d"][r0:r1] == 0.0)                # exactly zero ...
        if not flags & 1:
            assert np.array_equal(got["x"][r0:r1].view(np.int64), x[r0:r1].view(np.int64))   # ... and x bit-unchanged
    for v in bufs.values():
        v.free()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("with_dscale", [False, True])
def test_cheb_dir_against_numpy(lib, flags, with_dscale):
    for shift in (0, 1):
        run_cheb_dir(lib, flags, with_dscale, shift)
    with fused_off(lib):                                     # the composed form meets the same bar
        run_cheb_dir(lib, flags, with_dscale, 0)


# ---- 9. fused against composed --------------------------------------------------------------------------------------
def test_fused_equals_composed(lib, case20):
    """"cheb_fused" 0 replaces both kernels of the feature: k_cheb_dir by block_colscale / axpy / xmy / copy, and
    k_spmv_sell_res by bk::spmv + bk::axpy(r, -1, q).  The issue's bar is 1e-13 relative.  The code claims more, the same
    bits, and the claim follows from the arithmetic: the step is fl(fl(a z) + fl(b d)) in both forms (contraction off in
    cheb_dev.hip), and the residual is the row sum of bk::spmv, summed in its order, then ONE rounded subtraction
    r - sum in both (-1 q is exact, so axpy's r + (-1) q rounds once whether fused or not).  So equality is asserted."""
    mesh, dec, a, b = case20
    argv = argv_for("SRAS,1", "cg") + CHEB + ["-dls1_ksp_rtol", "1e-7"]
    x = np.random.default_rng(4).standard_normal(mesh.nbNode)
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    K = int(pc.local_solver_info()[2].max())
    y1 = pc.apply(x)
    c1 = pc.local_solver_counters()
    assert c1["K"] == K and c1["solves"] == 1 and c1["fused_residuals"] == K - 1      # k_spmv_sell_res took every update
    with fused_off(lib):
        y0 = pc.apply(x)                                     # same PC: the graph is recaptured for the other form
        c0 = pc.local_solver_counters()
        assert c0["solves"] == 2 and c0["fused_residuals"] == K - 1                   # ... and none of this solve's
        pc0 = cases.run_pc(lib, mesh, dec, argv, b)          # and a set-up that never saw the fused kernels
        y00 = pc0.apply(x)
        info0 = pc0.local_solver_info()
        assert pc0.local_solver_counters()["fused_residuals"] == 0
        pc0.destroy()
    err = np.linalg.norm(y1 - y0) / np.linalg.norm(y1)
    print("fused vs composed: %.3e relative (same PC), %.3e (own set-up)" % (err, np.linalg.norm(y1 - y00) / np.linalg.norm(y1)))
    assert err <= 1e-13 and np.linalg.norm(y1 - y00) <= 1e-13 * np.linalg.norm(y1)
    assert np.array_equal(y1, y0) and np.array_equal(y1, y00)
    assert np.array_equal(info0[2], pc.local_solver_info()[2])
    for i in range(4):
        assert np.array_equal(info0[i], pc.local_solver_info()[i])     # the verification solve ran composed: same bits
    pc.destroy()


# ---- 3 on the GPU: against the dense inverse, at the default precision ----------------------------------------------
def test_gpu_apply_equals_sum_of_dense_inverses(lib, case12):
    """The reference that does not depend on the host twin: Sum R^T A_Dir^-1 R x from numpy, against the GPU's apply at its
    default (single-precision companions in the V-cycle).  The bar is the one of the host test: -dls1_ksp_rtol 1e-10
    times a conditioning margin of 100 (the local matrices measure kappa = 133)."""
    mesh, dec, a, b = case12
    pc = cases.run_pc(lib, mesh, dec, argv_for("ASM,0") + CHEB + ["-dls1_ksp_rtol", "1e-10"], b)
    x = np.random.default_rng(3).standard_normal(mesh.nbNode)
    y = pc.apply(x)
    pc.destroy()
    ref = np.zeros(mesh.nbNode)
    for d in dec.domains:
        ref[d.l2g] += np.linalg.solve(d.a_dir.toarray(), x[d.l2g])
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print("12^3 on the GPU, default precision: |M x - sum R^T A_Dir^-1 R x| / |.| = %.3e" % err)
    assert err <= 1e-8


# ---- 10. the GPU against the host twin ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["default", "double"])
@pytest.mark.parametrize("which", ["dense12", "linear20"])
def test_gpu_equals_host_twin(lib, host, case12, case20, which, precision):
    """The applies of the dense-inverse case (12^3, ASM,0, 1e-10) and of the linearity case (20^3, SRAS,1, 1e-3) on the GPU
    and on the host twin: apply within 1e-10 relative, k_s and K equal -- at the default, which is what the GPU runs, and
    with -dls1_amg_precision double on both sides.
    The bounds bar, 1e-9 relative ("room for the V-cycle's summation orders"), is asserted on the double hierarchy only.
    The host twin has no single-precision companions (its csr_make_lp answers false), so its V-cycle always reads the FP64
    level matrices; at the GPU's default the two V-cycles are different operators (level matrices rounded to float, 6e-8
    relative per entry) and their extreme Ritz values differ by that rounding, not by summation order: measured on an
    MI355X at 20^3, 1.1e-8 (lo) and 2.2e-9 (hi) relative, with the applies at 3.9e-11.  There the bounds are printed.
    (At 12^3 the default and the double hierarchy gave the same figures, 7e-15 on the bounds and 2e-16 on the apply.)"""
    if which == "dense12":
        (mesh, dec, a, b), argv = case12, argv_for("ASM,0") + CHEB + ["-dls1_ksp_rtol", "1e-10"]
    else:
        (mesh, dec, a, b), argv = case20, argv_for("SRAS,1", "cg") + CHEB + ["-dls1_ksp_rtol", "1e-3"]
    if precision == "double":
        argv = argv + ["-dls1_amg_precision", "double"]
    x = np.random.default_rng(3).standard_normal(mesh.nbNode)
    res = []
    for l in (lib, host):
        pc = cases.run_pc(l, mesh, dec, argv, b)
        res.append((pc.apply(x), pc.local_solver_info(), pc.local_solver_table().shape[0]))
        pc.destroy()
    (yg, ig, kg), (yh, ih, kh) = res
    err = np.linalg.norm(yg - yh) / np.linalg.norm(yh)
    dlo, dhi = np.max(np.abs(ig[0] - ih[0]) / ih[0]), np.max(np.abs(ig[1] - ih[1]) / ih[1])
    print("%s, %s: apply %.3e relative, bounds lo %.3e hi %.3e relative, K = %d" % (which, precision, err, dlo, dhi, kg))
    assert np.array_equal(ig[2], ih[2]) and kg == kh
    if precision == "double":
        assert dlo <= 1e-9 and dhi <= 1e-9
    assert err <= 1e-10


# ---- 11. graph replay and re-set-up ---------------------------------------------------------------------------------
def test_graph_replay_and_resetup(lib, case20):
    mesh, dec, a, b = case20
    pc = cases.run_pc(lib, mesh, dec, argv_for("SRAS,1", "cg") + CHEB + ["-dls1_ksp_rtol", "1e-7"], b)
    K = int(pc.local_solver_info()[2].max())
    x = np.random.default_rng(8).standard_normal(mesh.nbNode)
    its0 = pc.info()["dls1_iterations"]
    first = pc.apply(x)                                      # direct launches (the graph is recorded next to them)
    assert pc.local_solver_counters() == dict(K=K, solves=1, graph_launches=0, fused_residuals=K - 1)
    for i in range(1, 30):                                   # replays
        assert np.array_equal(pc.apply(x), first), i
        assert pc.info()["dls1_iterations"] - its0 == K * (i + 1)
    assert pc.info()["dls1_solves"] == 30
    # what ran: 29 of the 30 solves came from the graph, and every residual update went through the fused sliced kernel
    assert pc.local_solver_counters() == dict(K=K, solves=30, graph_launches=29, fused_residuals=30 * (K - 1))
    table = pc.local_solver_table()
    pc.setup(b)                                              # releases the table and the graph, builds both again
    assert pc.local_solver_counters() == dict(K=K, solves=0, graph_launches=0, fused_residuals=0)
    assert np.array_equal(pc.local_solver_table(), table)
    assert np.array_equal(pc.apply(x), first)
    assert np.array_equal(pc.apply(x), first)
    assert pc.local_solver_counters() == dict(K=K, solves=2, graph_launches=1, fused_residuals=2 * (K - 1))
    pc.destroy()


# ---- 12. the full path ----------------------------------------------------------------------------------------------
def test_gmres_count_equals_the_cg_paths(lib, case20):
    mesh, dec, a, b = case20
    its = {}
    for typ, rtol in (("cg", "1e-12"), ("chebyshev", "1e-10")):
        pc = cases.run_pc(lib, mesh, dec, argv_for("RAS,1", "gmres", ["-ksp_rtol", "1e-8", "-dls1_ksp_type", typ, "-dls1_ksp_rtol", rtol]), b)
        x, its[typ], rnorm, reason = pc.solve(b)
        assert reason.startswith("KSP_CONVERGED")
        pc.destroy()
    print("20^3 RAS,1 GMRES on the GPU: cg %(cg)d, chebyshev %(chebyshev)d iterations" % its)
    assert its["chebyshev"] == its["cg"]
