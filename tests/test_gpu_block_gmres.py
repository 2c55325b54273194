"""-m gpu: block GMRES of KSPMatSolve_GenEO (-ksp_matsolve_type gmres) on the device, HIP library, no fallback: the checks
of tests/block_gmres_util.py that the host twin runs too -- the Gram-Schmidt kernels of csrc/block_dev.hip against
block_coldot and block_axpy_cols to the bit, the options, the block solve against KSPSolve_GenEO column by column with the
default restart and with -ksp_gmres_restart 5, -ksp_max_it --, then the kernels against their composed forms inside the
solve, and the GPU against the host twin."""
import pytest

import block_gmres_util as G
import block_rhs_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    lib = _lib.load()          # raises if the HIP library is missing: no fallback
    yield lib
    U.release_pcs(lib)


@pytest.fixture(scope="module")
def host():
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    yield lib
    U.release_pcs(lib)


def shapes(lib):
    g = G.gs_group(lib)
    return [(U.N_K, nb) for nb in (1, g, g + 1, 31)] + [(1, g + 1), (65537, 2)]


@pytest.mark.parametrize("w", [16, 32])
def test_gs_dots_equals_coldot_slab_by_slab(lib, w):
    for n, nb in shapes(lib):
        G.check_gs_dots(lib, w, n, nb)
    G.check_gs_dots(lib, w, U.N_K, G.gs_group(lib) + 1, composed=True)      # the composed form: same bits


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("norms", [True, False])
def test_gs_update_equals_successive_axpys(lib, w, norms):
    for n, nb in shapes(lib) + [(130, 65)]:            # 65 slabs: more than one launch of the kernel holds coefficients for
        G.check_gs_update(lib, w, n, nb, norms)
    G.check_gs_update(lib, w, U.N_K, G.gs_group(lib) + 1, norms, composed=True)


@pytest.mark.parametrize("w", [16, 32])
def test_scale_cols(lib, w):
    G.check_scale_cols(lib, w)
    G.check_scale_cols(lib, w, composed=True)


def test_options(lib):
    G.check_options(lib)


@pytest.mark.parametrize("lvl,n,w,seeds", G.CASES)
def test_block_gmres_equals_solve_column_by_column(lib, lvl, n, w, seeds):
    G.check_parity(lib, lvl, n, w, seeds)


@pytest.mark.parametrize("lvl,n,w,seeds", G.CASES)
def test_restarts_and_freezing(lib, lvl, n, w, seeds):
    G.check_restart_spread(lib, lvl, n, w, seeds)
    G.check_parity(lib, lvl, n, w, seeds, G.RESTART5)


def test_max_it(lib):
    G.check_max_it(lib, *G.CASES[0])


@pytest.mark.parametrize("extra,restart", [((), 30), (tuple(G.RESTART5), 5)])
def test_counters_and_composed_forms(lib, extra, restart):
    """GeneoSetKernelVariant("block_fused", 0): one block_coldot / block_axpy_cols per basis slab instead of the two
    Gram-Schmidt kernels -- X, its and rnorm to the bit, and the passes counted on the other side"""
    G.check_fused_against_composed(lib, *G.CASES[0], extra=list(extra), restart=restart)


@pytest.mark.parametrize("extra", [(), tuple(G.RESTART5)])
def test_gpu_equals_host_twin(lib, host, extra):
    import numpy as np
    lvl, n, w, seeds = G.CASES[0]
    B = G.solve_columns(n, tuple(seeds))
    argv = G.argv_for(lvl, w, list(extra))
    Xg, its_g, rn_g, rs_g = U.get_pc(lib, n, argv).mat_solve(B)
    Xh, its_h, rn_h, rs_h = U.get_pc(host, n, argv).mat_solve(B)
    err = U.relcols(Xg, Xh)
    print("block GMRES, GPU against host twin, %s %d^3 %s: its %s / %s, %.3e (bound %.1e)" % (
        lvl, n, list(extra), list(its_g), list(its_h), err, G.PARITY_BOUND))
    assert list(its_g) == list(its_h) and list(rs_g) == list(rs_h)
    assert np.isfinite(Xg).all() and err <= G.PARITY_BOUND
