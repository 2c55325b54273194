"""Right-preconditioned and flexible GMRES of KSPSolve_GenEO (-ksp_pc_side right, -ksp_type fgmres) on the host twin
(tests/hostsim): the composed forms of the two Gram-Schmidt primitives alone, the options, both methods against a numpy
reference with the default restart and with -ksp_gmres_restart 5, from a zero and from a random guess, the counters of
PCGenEOGetKrylovInfo, a preconditioner that changes between applications, and the left methods before and after.  The
checks live in tests/krylov_right_util.py and run unchanged on the GPU (tests/test_gpu_krylov_right.py)."""
import pytest

import block_rhs_util as U
import krylov_right_util as K


@pytest.fixture(scope="module")
def lib():
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    yield lib
    U.release_pcs(lib)


def test_options(lib):
    K.check_options(lib)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, K.BIG])
def test_vec_gs_dots(lib, n):
    assert n in K.sizes(lib)
    K.check_vec_dots(lib, n)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, K.BIG])
def test_vec_gs_update(lib, n):
    assert n in K.sizes(lib)
    K.check_vec_update(lib, n, composed=True)          # the host twin has the composed forms alone


@pytest.mark.parametrize("restart,guess", K.CONFIGS)
@pytest.mark.parametrize("lvl,n", K.CASES)
def test_against_the_numpy_reference(lib, lvl, n, restart, guess):
    K.check_case(lib, lvl, n, restart, guess)


def test_krylov_info(lib):
    K.check_krylov_info(lib, on_gpu=False)


@pytest.mark.parametrize("lvl,n", K.NONLINEAR)
def test_flexible_with_a_changing_preconditioner(lib, lvl, n):
    K.check_nonlinear(lib, lvl, n)


@pytest.mark.parametrize("lvl", ["RAS,1", "SRAS,1"])
def test_left_methods_are_not_disturbed(lib, lvl):
    K.check_disturbs_nothing(lib, lvl, 12)
