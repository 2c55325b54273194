"""-m gpu: the GenEO hot path on the MI355X (through the C ABI) against the oracle.

Bars (BASELINE.json north_star): Krylov iteration counts identical; eigenvalues within 1e-10
relative; number of retained eigenvectors / Nicolaides count exact; solution within 1e-8 of the
oracle's iterate at the same tolerance and within 1e-10 relative at ksp_rtol 1e-12.
"""
import numpy as np
import pytest

import cases
import dummy_cases as dc

pytestmark = pytest.mark.gpu

TIGHT = cases.TIGHT      # eigenpairs 1e-10; Krylov 1e-8 (GMRES) / 1e-6 (CG): see cases.Tight


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()


# The oracle's OWN PCG count of one mode case depends on the host it runs on: SRAS,1 / CG / overlap 2 meets rtol 1e-6 at
# iteration 24 or 25, and which one is decided by the summation order of the host's BLAS (OpenBLAS picks its kernels by
# CPU model and splits its loops by thread count): 24 with the Haswell or Zen kernels on one thread (iteration 23 at 1.17
# of the threshold), 25 with the SkylakeX or Sandybridge kernels or several threads.  The GPU's 25 is one of the oracle's
# own answers; this one pair is declared (cases.compare_with_oracle still compares the first residual norms to 1e-8 and
# records the case in cases.COUNT_DRIFT, printed in the terminal summary).  Every other count stays exact.
HOST_BLAS_DRIFT = {("SRAS,1", "cg", 2): [(25, 24)]}


@pytest.mark.parametrize("lvl,ksp,overlap", [("ASM,0", "cg", 1), ("ASM,1", "cg", 1), ("ASM,1", "gmres", 2),
                                             ("RAS,1", "gmres", 1), ("SRAS,1", "cg", 2), ("ASM,H1", "cg", 1),
                                             ("ASM,E1", "gmres", 1), ("SRAS,H1", "cg", 2), ("SRAS,1", "cg", 1),
                                             ("RAS,H1", "gmres", 2), ("ORAS,1", "gmres", 1)])
def test_modes_match_oracle(lib, lvl, ksp, overlap):
    argv = ["-geneo_lvl", lvl, "-geneo_tau", "0.2", "-geneo_cut", "8", "-ksp_type", ksp] + TIGHT
    cases.compare_with_oracle(lib, 12, (2, 2, 2), overlap, argv, count_drift=HOST_BLAS_DRIFT.get((lvl, ksp, overlap)))


@pytest.mark.parametrize("lvl,ksp,n,parts,cut,inter", [("SORAS,2", "cg", 12, (3, 2, 1), 12, True),
                                                       ("ORAS,H2", "gmres", 10, (2, 2, 2), 10, False),
                                                       ("SORAS,E2", "cg", 6, (2, 2, 1), 12, False),
                                                       ("SORAS,2", "cg", 16, (2, 2, 2), 14, False)])
def test_geneo2_matches_oracle(lib, lvl, ksp, n, parts, cut, inter):
    """GenEO-2 (geneo.cpp:1274-1300): tau problem on (A_Neu, A_Rob) with tau_loc and gamma problem on
    (D A_Dir D, A_Rob) with gamma_loc -- the largest eigenvalues, computed by LOBPCG on the inverted pencil."""
    argv = ["-geneo_lvl", lvl, "-geneo_tau", "0.02", "-geneo_gamma", "1.05", "-geneo_cut", str(cut), "-geneo_optim", "0.5",
            "-ksp_type", ksp] + TIGHT
    _, info = cases.compare_with_oracle(lib, n, parts, 1, argv, with_intersect=inter)
    assert info["dimE"] > len(parts)


def test_no_cut_keeps_every_eigenvalue_below_tau(lib):
    """No -geneo_cut: the reference's inertia count keeps every eigenvalue below tau; the LOBPCG block grows to reach it."""
    _, info = cases.compare_with_oracle(lib, 10, (2, 2, 2), 1, ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.42", "-ksp_type", "cg"] + TIGHT)
    assert info["dimE"] == 276


def test_geneo_chk_diagnostics_on_gpu(lib, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    argv = ["-geneo_lvl", "SORAS,2", "-geneo_tau", "0.02", "-geneo_gamma", "1.05", "-geneo_cut", "10", "-geneo_optim", "0.5",
            "-ksp_type", "cg", "-geneo_chk", "log"] + TIGHT
    _, info = cases.compare_with_oracle(lib, 10, (2, 2, 2), 1, argv)
    assert float((tmp_path / "check.SPD.A.log").read_text().splitlines()[0].split(":")[1]) > 0
    for gid in range(8):
        assert "nbNegEV 0, nbNullEV 0, nbPosEV 290" in (tmp_path / ("check%d.SPD.gamma.B.log" % gid)).read_text()
        r = np.loadtxt(tmp_path / ("check%d.setup.Z.R" % gid))
        assert np.all(np.abs(np.diag(r)) > 1e-8)
    assert np.loadtxt(tmp_path / "check.setup.ZE2G.R").shape == (info["dimE"], info["dimE"])


def test_config0_laplacian_2d_two_subdomains_five_vectors(lib):
    """BASELINE configs[0]: tst/laplacian 2-D stencil, 2 subdomains, 5 eigenvectors per subdomain."""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.9", "-geneo_cut", "5", "-ksp_type", "gmres"] + TIGHT
    its, info = cases.compare_with_oracle(lib, 40, (2, 1, 1), 1, argv, dim=2, gen=dict(kappa_max=2.0, interp="lin"))
    assert info["dimE"] == 10


@pytest.mark.parametrize("no_ground", [True, False])
def test_config4_graph_irregular_csr(lib, no_ground):
    """BASELINE configs[4] in small: tst/graph generator (with the ground node the matrix has one very
    long row -> long-row SpMV kernel), node-range partition, 4 subdomains."""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.3", "-geneo_cut", "6", "-ksp_type", "cg"] + TIGHT
    cases.compare_with_oracle(lib, 0, None, 1, argv, case=cases.graph_case(size=400, level=2, nb=4, overlap=1,
                                                                           no_ground=no_ground))


def test_dirichlet_built_by_library(lib):
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.2", "-geneo_cut", "8", "-ksp_type", "cg"] + TIGHT
    cases.compare_with_oracle(lib, 12, (2, 2, 2), 1, argv, with_dir=False)


def test_variable_kappa_and_uneven_parts(lib):
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.15", "-geneo_cut", "12", "-ksp_type", "cg"] + TIGHT
    cases.compare_with_oracle(lib, 14, (3, 2, 1), 1, argv, gen=dict(kappa_max=4.0, interp="lin"))


def test_heat_high_contrast(lib):
    """BASELINE config 4: GenEO coarse space vs plain ASM on the high-contrast heat operator (kappa = 100 on the middle
    third of every axis: contrast 100^3 = 1e6).

    Rounds 1-2 compared the coarse action here to 1e-7 "because E inherits the conditioning of A".  It does not:
    cond(E) is ~2e2 (asserted below) and the dense E-solve is exact to 1e-15.  What limits the comparison is the
    contrast itself: eigenvectors are normalised and converged in the B-inner product (B = D A_Dir D carries the
    coefficient), so their components in the kappa = 1 regions weigh 1e-6 of those in the kappa = 1e6 region and are
    resolved to eps * contrast = 2e-10 relative to the vector -- and Q b is compared in the 2-norm, which weighs all
    components alike.  Any solver working in that inner product (ARPACK's shift-invert too) has this floor.  The bar is
    therefore 100 eps contrast = 2.2e-8 for the operator actions of the two-level case, asserted together with
    cond(E); the one-level case keeps the suite's 1e-9."""
    contrast = 100.0 ** 3
    gen = dict(heat=True, kappa_max=100.0, interp="minmax")
    a0 = ["-geneo_lvl", "ASM,0", "-ksp_type", "cg"] + TIGHT
    a1 = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.015", "-geneo_cut", "12", "-ksp_type", "cg"] + TIGHT
    its0, _ = cases.compare_with_oracle(lib, 12, (2, 2, 2), 1, a0, gen=gen)
    its1, _ = cases.compare_with_oracle(lib, 12, (2, 2, 2), 1, a1, gen=gen, aptol=100 * np.finfo(float).eps * contrast)
    assert its1 <= its0
    mesh, dec, a, b = cases.grid_case(n=12, dim=3, parts=(2, 2, 2), overlap=1, **gen)
    pc = cases.run_pc(lib, mesh, dec, a1, b)
    e = pc.E()
    assert np.linalg.cond(e) < 1e3                     # the coarse operator is NOT the ill-conditioned object
    zb = np.random.default_rng(0).random(e.shape[0])
    assert np.linalg.norm(e @ np.linalg.solve(e, zb) - zb) <= 1e-13 * np.linalg.norm(zb)
    pc.destroy()


def test_solution_1e10(lib):
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.2", "-geneo_cut", "8", "-ksp_type", "cg",
            "-els2_eps_tol", "1e-9", "-ksp_rtol", "1e-12", "-ksp_atol", "1e-50"]
    mesh, dec, a, b = cases.grid_case(12, 3, (2, 2, 2), 1)
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    x, its, rnorm, reason = pc.solve(b)
    exact = np.arange(1.0, mesh.nbNode + 1.0)
    assert np.linalg.norm(x - exact) <= 1e-10 * np.linalg.norm(exact)


@pytest.mark.parametrize("lvl,ksp", [("SRAS,1", "cg"), ("RAS,1", "gmres")])
def test_converged_solution_matches_the_oracles_to_1e10_at_the_bench_options(lib, lvl, ksp):
    """north_star: "eigenvalues and solution within 1e-10 relative".  The bench's own option set (overlap 2, -geneo_cut 20,
    tau 0.35, AMG inside the local solves and LOBPCG) on 24^3 in 8 subdomains with both Krylov loops driven to
    convergence (-ksp_rtol 1e-13): the library's solution against the ORACLE's (exact LU, exact eigenpairs) -- two
    converged solves of the same system -- and against the analytic one (1, 2, .., N), all within 1e-10 relative."""
    import oracle.geneo_oracle as go
    argv = cases.bench_argv(["-geneo_lvl", lvl, "-ksp_type", ksp, "-ksp_rtol", "1e-13", "-ksp_gmres_restart", "200",
                             "-els2_eps_tol", "1e-10", "-dls1_ksp_rtol", "1e-12"])
    mesh, dec, a, b = cases.grid_case(24, 3, (2, 2, 2), cases.BENCH_OVERLAP)
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    x, its, rnorm, reason = pc.solve(b)
    assert reason.startswith("KSP_CONVERGED"), reason
    orc = cases.oracle_for(mesh, dec, argv, b)
    kspname, kw = cases.ksp_args(argv)
    res = go.solve(orc, b, kspname, **kw)
    exact = np.arange(1.0, mesh.nbNode + 1.0)
    assert np.linalg.norm(res.x - exact) <= 1e-10 * np.linalg.norm(exact)
    assert np.linalg.norm(x - exact) <= 1e-10 * np.linalg.norm(exact)
    assert np.linalg.norm(x - res.x) <= 1e-10 * np.linalg.norm(res.x)
    for s in range(8):
        np.testing.assert_allclose(np.sort(pc.eigenvalues(s)), np.sort(orc.eigvals[s]), rtol=1e-10, atol=1e-13)
    pc.destroy()


@pytest.mark.parametrize("rec", dc.geneo_refs(),
                         ids=lambda r: r["file"][:-4])
def test_dummy_goldens_on_gpu(lib, rec):
    """The reference's own tst/dummy goldens -- all 80 GenEO rows: ASM,0/1/H1/E1 and SORAS,0/2/H2/E2 -- through the HIP
    library: local matrices in, converged solution out (to PETSc print precision)."""
    from geneo4petsc_amd import decomp
    from geneo4petsc_amd.pc import GenEOPC
    d = dc.load()
    mesh = decomp.read_input_text(d["inputs"][rec["input"] + ".inp"], rec["inpEps"])
    ep, npart = dc.partition_for(rec)
    dec = decomp.decompose(mesh, 2, ep, npart, rec["metis"] == "dual", rec["overlap"])
    for p in range(2):
        assert dc.same_rows(dc.rows_of(dec.domains[p].a_neu), rec["mats"][p])
    a = decomp.global_matrix(mesh)
    b = decomp.read_b_text(d["inputs"]["B.inp"], mesh.nbNode) if rec["use_b_file"] else decomp.rhs_default(a)
    np.testing.assert_allclose(b, rec["b"], rtol=1e-6)
    argv = ["-geneo_lvl", rec["geneo_lvl"], "-ksp_rtol", "1e-12", "-ksp_atol", "1e-12"]
    if rec["geneo_cut"] > 0:
        argv += ["-geneo_cut", str(rec["geneo_cut"])]
    pc = GenEOPC(lib)
    pc.set_from_options(argv)
    assert ("INFO: %s pc" % pc.name) in rec["info"][2]
    pc.set_sizes(mesh.nbNode, 2)
    for dom in dec.domains:
        pc.add_subdomain(dom.gid, dom.l2g, dom.mult, dom.a_neu, None)
    pc.setup(b)
    x, its, rnorm, reason = pc.solve(b)
    assert reason.startswith("KSP_CONVERGED")
    np.testing.assert_allclose(x, rec["x"], rtol=1e-5, atol=1e-6)


def test_hub_row_falls_back_to_host_products(lib, capfd, monkeypatch):
    """A hub node tied to 300 scattered grid nodes: its row of A P has more than 256 distinct columns, the device
    sparse product reports the overflow, the partly built hierarchy is dropped and the host products take over --
    same answer as the oracle."""
    from geneo4petsc_amd import decomp
    nx = 40
    idx = lambda i, j: i + nx * j
    ptr, elems, mats = [0], [], []
    e2 = [1.0001, -1.0, -1.0, 1.0001]
    for j in range(nx):
        for i in range(nx):
            if i + 1 < nx:
                elems += [idx(i, j), idx(i + 1, j)]; ptr.append(len(elems)); mats.append(e2)
            if j + 1 < nx:
                elems += [idx(i, j), idx(i, j + 1)]; ptr.append(len(elems)); mats.append(e2)
    hub = nx * nx
    rng = np.random.default_rng(5)
    for t in rng.choice(nx * nx, size=300, replace=False):
        elems += [int(t), hub]; ptr.append(len(elems)); mats.append([0.0101, -0.01, -0.01, 0.0101])
    mesh = decomp.mesh_from_lists(hub + 1, ptr, elems, mats)
    npart = (np.arange(hub + 1) >= (hub + 1) // 2).astype(np.int64)
    dec = decomp.decompose(mesh, 2, None, npart, False, 1)
    a = decomp.global_matrix(mesh)
    b = decomp.rhs_default(a)
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.05", "-geneo_cut", "6", "-ksp_type", "cg", "-amg_coarse_size", "200"] + TIGHT
    monkeypatch.setenv("GENEO_DEBUG", "1")
    cases.compare_with_oracle(lib, 0, None, 1, argv, case=(mesh, dec, a, b), aptol=1e-8)
    err = capfd.readouterr().err
    assert "A_Neu hierarchy (host products)" in err


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("post", ["1", ""])
def test_vcycle_storage_and_form_do_not_change_the_result(lib, precision, post, monkeypatch):
    """The local solves' V-cycle with FP64 level matrices (-dls1_amg_precision double) or their single-precision
    companions (default), with the one-product post-smoothing (M = P - w D^-1 A P, default) or the two-launch form
    (GENEO_AMG_NO_POST_MATRIX): the same iteration counts as the oracle and the same solution in all four, on a case
    whose subdomains are large enough for a three-level hierarchy (20^3 in 8 subdomains, AMG inner solves)."""
    if post:
        monkeypatch.setenv("GENEO_AMG_NO_POST_MATRIX", post)
    # Round 2 saw GMRES(30) stop after 33 iterations here where the oracle needs 32 (gpurun_out/s2.log) and answered by
    # loosening the test.  The cause, isolated in round 3 on the same argv (tests/test_oracle_eig.py::
    # test_gmres_count_at_1e8_moves_with_a_1e10_perturbation_of_the_oracle_itself): NOT the inexact local solves
    # (-dls1_ksp_rtol 1e-14 and -dls1_pc_type jacobi give the same 33) and NOT a cut inside a multiplet (cut 12 takes the
    # whole doublet 0.204296.. of the corner subdomains; the near-triplet 0.20584377 / ..77 / ..82 of the others is split
    # 5e-8 apart), but the eigenvectors: converged to 1e-10 they perturb Z E^-1 Z^T by 1e-10, and the ORACLE ITSELF, with
    # its preconditioner perturbed by a fixed relative 1e-10 (1e-12), needs 33 (34) iterations instead of 32 at rtol 1e-8
    # -- by iteration 18 two Krylov processes whose operators differ by 1e-10 are no longer the same sequence.  With the
    # eigenvectors at 1e-12 the library reproduces the oracle's 32; the original parameters are restored with that.
    argv = ["-geneo_lvl", "SRAS,1", "-geneo_tau", "0.35", "-geneo_cut", "12", "-ksp_type", "gmres", "-dls1_pc_type", "amg",
            "-els2_pc_type", "amg", "-dls1_amg_precision", precision, "-amg_coarse_size", "100"] + TIGHT + ["-els2_eps_tol", "1e-12"]
    _, info = cases.compare_with_oracle(lib, 20, (2, 2, 2), 2, argv)
    assert info["amg_levels"] >= 3


@pytest.mark.parametrize("span_max", ["250", "60"])
def test_two_base_and_32bit_column_layouts_of_the_companions_in_a_solve(lib, span_max, monkeypatch, capfd):
    """The single-precision companions of the V-cycle with their 16-bit column offsets limited to a span of 250 (the
    12^3 blocks' slices span 352 columns: two bases per slice, as a 187^3 block's do at the real limit of 65535) and of
    60 (32-bit columns kept): same counts as the oracle, same solution."""
    monkeypatch.setenv("GENEO_LP_SPAN_MAX", span_max)
    monkeypatch.setenv("GENEO_DEBUG", "1")
    argv = ["-geneo_lvl", "SRAS,1", "-geneo_tau", "0.35", "-geneo_cut", "12", "-ksp_type", "gmres", "-dls1_pc_type", "amg",
            "-els2_pc_type", "amg", "-amg_coarse_size", "100"] + TIGHT + ["-els2_eps_tol", "1e-12"]
    cases.compare_with_oracle(lib, 20, (2, 2, 2), 2, argv)
    err = capfd.readouterr().err
    assert ("slices with two column bases" if span_max == "250" else "32-bit columns kept") in err


def test_large_coarse_operator_blocked_cholesky(lib):
    """dimE = 312 and a 64-column LOBPCG block (192-column Gram / block update kernels); E through the blocked Cholesky."""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.9", "-geneo_cut", "39", "-ksp_type", "cg"] + TIGHT
    _, info = cases.compare_with_oracle(lib, 12, (2, 2, 2), 1, argv)
    assert info["dimE"] == 312


@pytest.mark.parametrize("style", ["PCGenEOSetup", "initGenEOPC"])
def test_reference_style_entry_points(lib, style):
    """hdr/geneo_c.h:10 PCGenEOSetup (after KSPSetOperators with the MATIS view) and hdr/geneo.hpp:30 initGenEOPC:
    one subdomain for this rank; with ASM,1 on a single subdomain the pencil (A, A) has only eigenvalue 1, so Z is the
    empty-Z rule's constant vector (geneo.cpp:1305-1314) and M^-1 = A^-1 + Q."""
    from geneo4petsc_amd import decomp
    from geneo4petsc_amd.pc import GenEOPC
    mesh = decomp.grid_mesh(size=8, dim=3)
    a = decomp.global_matrix(mesh).tocsr()
    n = a.shape[0]
    b = decomp.rhs_default(a)
    pc = GenEOPC(lib)
    pc.set_from_options(["-geneo_lvl", "ASM,1", "-ksp_type", "cg", "-ksp_rtol", "1e-10"])
    if style == "PCGenEOSetup":
        pc.setup_from_operators(n, np.arange(n), a, np.ones(n, dtype=np.int32), None, [np.zeros(0, dtype=np.int32)])
    else:
        pc.init(n, n, np.arange(n), a, None, None, None, np.arange(n), np.ones(n, dtype=np.uint32), [[]])
    pc.setup(b)
    info = pc.info()
    assert info["dimE"] == 1 and info["nicolaidesLoc"] == 1
    x, its, rnorm, reason = pc.solve(b)
    assert reason.startswith("KSP_CONVERGED") and its <= 4
    np.testing.assert_allclose(x, np.arange(1.0, n + 1.0), rtol=1e-7)
    one = np.ones(n)
    q = one * (one @ b) / (one @ (a @ one))
    np.testing.assert_allclose(pc.apply(b), np.arange(1.0, n + 1.0) + q, rtol=1e-7)
    pc.destroy()


@pytest.mark.parametrize("lvl,tau,dim_e", [("ASM,1", "0.6", 1256), ("SRAS,1", "0.5", None)])
def test_no_cut_deflated_restarts(lib, lvl, tau, dim_e):
    """Row a7: every eigenvalue below tau enters Z, for any count (geneo.cpp:502-560, :713) -- 16^3 in 8 subdomains of
    729 rows, no -geneo_cut: 157 vectors per subdomain at tau 0.6 (four deflated restarts behind the 64-column block),
    on LOBPCG-sized subdomains (the dense host path stops at 192 rows).  dimE, kept counts, eigenvalues to 1e-10 and the
    GMRES count equal the oracle's."""
    argv = ["-geneo_lvl", lvl, "-geneo_tau", tau, "-ksp_type", "gmres"] + TIGHT
    _, info = cases.compare_with_oracle(lib, 16, (2, 2, 2), 1, argv)
    assert info["dimE"] >= 8 * 70
    if dim_e:
        assert info["dimE"] == dim_e


def test_singular_neumann_matrices_get_null_pivot_fixing(lib):
    """--inpEps 0 (see tests/test_hostsim.py, same name): null pivots of the singular Neumann blocks are detected and
    fixed as the reference asks of MUMPS (tuneSolver, geneo.cpp:76-92); 20^3 so that the hierarchies have three levels."""
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.2", "-geneo_cut", "8", "-ksp_type", "gmres", "-amg_coarse_size", "100"] + TIGHT
    info = cases.check_singular_neumann_case(lib, 20, argv)
    assert info["amg_levels"] >= 3


@pytest.mark.parametrize("lvl,ksp,overlap", [("SRAS,1", "cg", 2), ("RAS,1", "gmres", 1), ("ASM,H1", "cg", 1)])
def test_cooperative_reductions_of_large_subdomains(lib, lvl, ksp, overlap):
    """The one-subdomain-per-GPU layout of the benchmark's configuration has thousands of 1024-row chunks per subdomain:
    above GENEO_PAR_REDUCE_MIN chunks the per-subdomain reductions (the batched PCG's scalars, Z^T x, the Gram partials)
    run cooperatively -- one workgroup per subdomain, once per launch (k_sub_totals, k_zt_reduce_big, k_gram_reduce_z).
    Forced here on small cases (threshold 0): full parity with the oracle, and the same counts as the default forms."""
    argv = ["-geneo_lvl", lvl, "-geneo_tau", "0.2", "-geneo_cut", "8", "-ksp_type", ksp] + TIGHT
    n, parts = 12, (2, 2, 2)          # the cases of test_modes_match_oracle
    drift = HOST_BLAS_DRIFT.get((lvl, ksp, overlap))
    its_default, info_default = cases.compare_with_oracle(lib, n, parts, overlap, argv, count_drift=drift)
    old = lib.GeneoSetParReduceMin(0)
    try:
        assert lib.GeneoSetParReduceMin(0) == 0
        its, info = cases.compare_with_oracle(lib, n, parts, overlap, argv, count_drift=drift)
    finally:
        lib.GeneoSetParReduceMin(old)
    assert its == its_default and info["dimE"] == info_default["dimE"]


def test_local_solves_single_step_tail(lib, monkeypatch):
    """Inner PCG of the local solves: behind the long first chunk the iteration goes on in pairs, or -- large subdomains --
    in single steps (HIP graphs per chunk length AND rz parity).  The row bound of the single steps is lowered so that a
    40^3 case takes them: the same outer iteration count, the same solution to the inner tolerance, and never more inner
    iterations than with pairs."""
    mesh, dec, a, b = cases.grid_case(n=40, dim=3, parts=(2, 2, 2), overlap=2)
    res = []
    for rows in ("1000000000", "1"):
        monkeypatch.setenv("GENEO_DLS1_SINGLE_STEP_ROWS", rows)
        pc = cases.run_pc(lib, mesh, dec, cases.bench_argv(), b)
        x, its, rnorm, reason = pc.solve(b)
        res.append((x, its, reason, pc.info()["dls1_iterations"]))
        pc.destroy()
    (x2, its2, r2, inner2), (x1, its1, r1, inner1) = res
    assert r1.startswith("KSP_CONVERGED") and its1 == its2
    assert inner1 <= inner2, (inner1, inner2)
    assert np.linalg.norm(x1 - x2) <= 1e-5 * np.linalg.norm(x2)
    print("inner PCG iterations of the solve: %d in pairs, %d in single steps behind the long chunk" % (inner2, inner1))


def test_eigensolve_coarse_start_nested(lib, monkeypatch, capfd):
    """VERDICT r3 item 8 (cut LOBPCG's iterations): -geneo_eig_coarse_start -- the fine eigensolve starts from the prolonged
    Ritz vectors of the level-1 Galerkin pencil, that solve from level 2 (nested iteration; the row bound of the nesting is
    lowered so that a 64^3 grid reaches it).  At a tight tolerance: the eigenvalues of the random start to 1e-8, the same
    kept counts, dimE and PCG count.  (What it buys is measured at 6.5 M rows per subdomain: 19 -> 7 fine iterations,
    profiles/r04_coarse_start_ab.log; below ~0.5 M rows it does not pay and the default threshold keeps it out.)"""
    monkeypatch.setenv("GENEO_COARSE_START_MIN_ROWS", "1")
    monkeypatch.setenv("GENEO_DEBUG", "1")
    off, on, worst = cases.check_coarse_start(lib, n=64)
    err = capfd.readouterr().err
    assert "[coarse start] level 2" in err and "[coarse start] level 1" in err and "not used" not in err
    assert on["dimE"] == 160
    print("coarse start at 64^3: %d coarse + %d fine LOBPCG iterations (random start: %d), worst relative eigenvalue difference %.1e"
          % (on["eigCoarseIterations"], on["eig_iterations"], off["eig_iterations"], worst))


def test_memory_bounded_setup_groups_give_the_ungrouped_result(lib):
    """the rank's subdomains eigensolved in consecutive groups under a device-memory budget
    (-geneo_eig_group_rows; what lets 368^3 in 8 subdomains fit ONE GPU) at the bench's own options: kept counts, dimE,
    the LOBPCG iteration count and the PCG count identical to the all-at-once path, eigenvalues within 1e-10 relative
    (cases.check_grouped_eigensolve says why not to the bit on the device)."""
    runs, worst = cases.check_grouped_eigensolve(lib, n=40, group_rows=(1, 30000), exact=False)
    assert runs[0]["info"]["dimE"] == 160
    print("grouped against all-at-once eigensolve, worst relative differences:", worst)
