"""Block GMRES of KSPMatSolve_GenEO (-ksp_matsolve_type gmres) on the host twin (tests/hostsim): the composed forms of its
Gram-Schmidt primitives alone, the options, the block solve against KSPSolve_GenEO column by column with the default restart
and with -ksp_gmres_restart 5, -ksp_max_it, and the counters of PCGenEOGetBlockKrylovInfo.  The checks live in
tests/block_gmres_util.py and run unchanged on the GPU (tests/test_gpu_block_gmres.py)."""
import pytest

import block_gmres_util as G
import block_rhs_util as U


@pytest.fixture(scope="module")
def lib():
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


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("norms", [True, False])
def test_gs_update_equals_successive_axpys(lib, w, norms):
    for n, nb in shapes(lib) + [(130, 65)]:            # 65 slabs: more than one launch of the kernel holds coefficients for
        G.check_gs_update(lib, w, n, nb, norms)


@pytest.mark.parametrize("w", [16, 32])
def test_scale_cols(lib, w):
    G.check_scale_cols(lib, w)


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
    G.check_fused_against_composed(lib, *G.CASES[0], extra=list(extra), restart=restart)

