"""Flexible CG of KSPSolve_GenEO (-ksp_type fcg) on the host twin (tests/hostsim): the options, the composed form of the step
primitive alone, the method against a numpy reference from a zero and from a random guess under both norm types, the
truncation window on a non-symmetric preconditioner, fcg against the library's cg on a fixed symmetric preconditioner, a
preconditioner that changes between applications, the counters of PCGenEOGetFcgInfo, and cg and gmres before and after.
The checks live in tests/fcg_util.py and run unchanged on the GPU (tests/test_gpu_fcg.py)."""
import pytest

import block_rhs_util as U
import fcg_util as F
import krylov_right_util as K


@pytest.fixture(scope="module")
def lib():
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    yield lib
    U.release_pcs(lib)


def test_options(lib):
    F.check_options(lib)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, K.BIG])
def test_vec_fcg_step(lib, n):
    assert n in K.sizes(lib)
    F.check_fcg_step(lib, n, composed=True)            # the host twin has the composed form alone


@pytest.mark.parametrize("guess,norm", F.CONFIGS)
@pytest.mark.parametrize("lvl,n", F.CASES)
def test_against_the_numpy_reference(lib, lvl, n, guess, norm):
    F.check_case(lib, lvl, n, guess, norm)


@pytest.mark.parametrize("mmax,trunc", F.TRUNC)
def test_truncation(lib, mmax, trunc):
    F.check_truncation(lib, mmax, trunc)


def test_the_window_matters_in_the_reference(lib):
    F.check_window_matters(lib)


@pytest.mark.parametrize("guess", [0, 1])
@pytest.mark.parametrize("lvl,n", F.EQUALS_CG)
def test_fcg_equals_cg_on_a_fixed_symmetric_preconditioner(lib, lvl, n, guess):
    F.check_equals_cg(lib, lvl, n, guess)


def test_fcg_against_cg_on_sras_is_reported(lib):
    """SRAS,1: measured and printed only (the histories of cg and fcg part by 1e-8 to 1e-6 of the first norm there)"""
    for guess in (0, 1):
        F.measure_equals_cg(lib, "SRAS,1", 12, guess)


@pytest.mark.parametrize("lvl,n", F.NONLINEAR)
def test_flexible_with_a_changing_preconditioner(lib, lvl, n):
    F.check_nonlinear(lib, lvl, n)


def test_counters(lib):
    F.check_counters(lib, on_gpu=False)


def test_other_methods_are_not_disturbed(lib):
    F.check_disturbs_nothing(lib, "SRAS,1", 12)
