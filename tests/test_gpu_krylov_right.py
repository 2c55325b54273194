"""-m gpu: right-preconditioned and flexible GMRES of KSPSolve_GenEO (-ksp_pc_side right, -ksp_type fgmres) on the device,
HIP library, no fallback: the checks of tests/krylov_right_util.py that the host twin runs too -- the Gram-Schmidt kernels
of csrc/krylov_dev.hip (fused: numpy's separately rounded arithmetic to the bit, the dots within the derived bound and
independent of alignment, width and position; composed under GeneoSetKernelVariant("krylov_fused", 0): within the derived
bounds), the options, both methods against the numpy reference, the counters, a preconditioner that changes between
applications, and the left methods before and after."""
import pytest

import block_rhs_util as U
import krylov_right_util as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    lib = _lib.load()          # raises if the HIP library is missing: no fallback
    yield lib
    U.release_pcs(lib)


def test_options(lib):
    K.check_options(lib)


@pytest.mark.parametrize("composed", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, K.BIG])
def test_vec_gs_dots(lib, n, composed):
    assert n in K.sizes(lib)
    K.check_vec_dots(lib, n, composed=composed)


@pytest.mark.parametrize("composed", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, K.BIG])
def test_vec_gs_update(lib, n, composed):
    assert n in K.sizes(lib)
    K.check_vec_update(lib, n, composed=composed)


@pytest.mark.parametrize("restart,guess", K.CONFIGS)
@pytest.mark.parametrize("lvl,n", K.CASES)
def test_against_the_numpy_reference(lib, lvl, n, restart, guess):
    K.check_case(lib, lvl, n, restart, guess)


def test_krylov_info(lib):
    K.check_krylov_info(lib, on_gpu=True)


@pytest.mark.parametrize("lvl,n", K.NONLINEAR)
def test_flexible_with_a_changing_preconditioner(lib, lvl, n):
    K.check_nonlinear(lib, lvl, n)


@pytest.mark.parametrize("lvl", ["RAS,1", "SRAS,1"])
def test_left_methods_are_not_disturbed(lib, lvl):
    K.check_disturbs_nothing(lib, lvl, 12)
