"""The coarse-device options and hooks on the host twin (tests/hostsim): a backend without the blocked coarse kernels
(coarse_dev.h) answers "not available", and the PC then runs the host sequence -- whatever -geneo_coarse_device asks."""
import ctypes as C

import numpy as np
import pytest

import cases
from hostsim_util import hostsim_lib

ARGV = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.2", "-geneo_cut", "4", "-els2_eps_tol", "1e-9", "-ksp_type", "cg",
        "-ksp_rtol", "1e-8"]


@pytest.fixture(scope="module")
def lib():
    return hostsim_lib()


@pytest.fixture(scope="module")
def case():
    return cases.grid_case(n=8, parts=(2, 2, 2), overlap=1)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_hooks_answer_not_available(lib):
    n = 5
    a = np.eye(n) * 4.0
    lo, lt, y = np.zeros((n, n)), np.zeros((n, n)), np.ones(n)
    st = C.c_int(7)
    assert lib.GeneoTestCoarseFactor(n, 16, _p(a), _p(lo), _p(lt), C.byref(st)) == -3
    assert not lo.any() and not lt.any()
    assert lib.GeneoTestCoarseSolve(n, 16, _p(a), _p(a), _p(y), 1) == -3
    assert np.array_equal(y, np.ones(n))


@pytest.mark.parametrize("key,value,word", [("-geneo_coarse_device", "bogus", "bogus"), ("-geneo_coarse_block", "17", "17"),
                                             ("-geneo_coarse_block", "0", "0"), ("-geneo_coarse_block", "272", "272")])
def test_bad_values_are_refused(lib, key, value, word):
    from geneo4petsc_amd.pc import GenEOPC, GenEOError
    pc = GenEOPC(lib)
    with pytest.raises(GenEOError) as e:
        pc.set_from_options(ARGV + [key, value])
    assert key in str(e.value) and word in str(e.value)
    pc.destroy()


def test_good_values_are_accepted_and_documented(lib):
    from geneo4petsc_amd.pc import GenEOPC
    pc = GenEOPC(lib)
    for dev in ("auto", "never", "always"):
        pc.set_from_options(ARGV + ["-geneo_coarse_device", dev, "-geneo_coarse_block", "48"])
    assert "-geneo_coarse_device" in pc.usage() and "-geneo_coarse_block" in pc.usage()
    pc.destroy()


def test_always_falls_back_to_the_host_sequence(lib, case):
    """`always` on a backend without the kernels: host factor, host round trip in the apply, and -- the host sweeps and
    the twin's chol_solve being the same loops -- the bits of the run without the option"""
    mesh, dec, a, b = case
    res = []
    for extra in ([], ["-geneo_coarse_device", "always", "-geneo_coarse_block", "16"], ["-geneo_coarse_device", "never"]):
        pc = cases.run_pc(lib, mesh, dec, ARGV + extra, b)
        ci = pc.coarse_info()
        q = pc.apply_q(b)
        x, its, rnorm, reason = pc.solve(b)
        assert reason.startswith("KSP_CONVERGED")
        res.append((ci, q, x, its, np.array(pc.residual_history())))
        pc.destroy()
    plain, always, never = res
    dim = plain[0][0]
    assert dim > 0
    assert plain[0] == (dim, 0, 1, 0) and never[0] == plain[0]      # default and never: host factor, one-workgroup sweeps
    assert always[0] == (dim, 0, 0, 0)                               # no device factor: host round trip
    for other in (always, never):
        assert other[3] == plain[3]
        assert np.array_equal(other[1], plain[1]) and np.array_equal(other[2], plain[2])
        assert np.array_equal(other[4], plain[4])
