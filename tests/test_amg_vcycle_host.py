"""The multigrid hierarchy and its V-cycle on the host twin (tests/hostsim) against the longdouble reference of
amg_cases.py: every form of the cycle, the set-up against scipy, independence of a subdomain's cycle from its batch.
The twin runs AmgDevice as it stands over the serial backend; it has no single-precision companions and no ragged-row
kernels, so those checks live in test_gpu_amg_vcycle.py only.  The figures are printed (pytest -s)."""
import numpy as np
import pytest

import amg_cases as ac
from hostsim_util import hostsim_lib


@pytest.fixture(scope="module")
def lib():
    return hostsim_lib()


@pytest.fixture(scope="module")
def blocks():
    return ac.make_blocks()


@pytest.fixture(scope="module")
def batch(blocks):
    return ac.batch_of(blocks)


def test_the_matrix_is_the_one_described(blocks, batch):
    a, suboff = batch
    assert list(np.diff(suboff)) == [1320, 210, 729, 18] and a.shape[0] == 2277
    assert all(int(o) % 64 for o in suboff[1:])
    assert np.diff(suboff)[-1] < ac.COARSE_SIZE
    assert abs(a - a.T).max() == 0 and np.all(a.diagonal() > 0)
    rho_s = ac.gershgorin(a, suboff, np.float64)[2]
    assert len(set(rho_s)) == 4                     # every block has its own Gershgorin bound: dinv is rescaled in three
    assert rho_s[0] < 0.95 * rho_s.max()            # ... and the first block's visibly so


@pytest.mark.parametrize("name", list(ac.CYCLE_CASES))
def test_cycle_against_reference(lib, monkeypatch, batch, name):
    a, suboff = batch
    nlev, err, err64, _ = ac.run_cycle_case(lib, monkeypatch, name, a, suboff, "hostsim")
    # the float64 evaluation of the reference stays an order of magnitude under the bound that is derived from it
    # (printed above; numpy's float64 summation order, and with it the exact figure, may differ between CPUs)
    assert err64 <= ac.CYCLE_BOUND / 10
    assert err <= ac.CYCLE_BOUND


@pytest.mark.parametrize("setup", ["device", "host"])
def test_hierarchy_against_scipy(lib, monkeypatch, batch, setup):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    H = ac.Hierarchy(lib, a, suboff, setup=setup)
    try:
        assert H.nlevels >= 3
        ac.assert_identities(H, a, "hostsim/" + setup)
    finally:
        H.destroy()


def test_device_and_host_setups_agree(lib, monkeypatch, batch):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    Hd = ac.Hierarchy(lib, a, suboff, setup="device")
    Hh = ac.Hierarchy(lib, a, suboff, setup="host")
    try:
        ac.assert_same_hierarchy(Hd, Hh, a, "hostsim")
    finally:
        Hd.destroy()
        Hh.destroy()


@pytest.mark.parametrize("degree", [1, 2])
def test_cycle_does_not_depend_on_the_batch(lib, monkeypatch, blocks, batch, degree):
    ac.set_env(monkeypatch, {})
    ac.check_batch_independence(lib, blocks, batch, degree, "hostsim")


def test_hook_reports_errors(lib, monkeypatch, batch):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    H = ac.Hierarchy(lib, a, suboff, setup="device", max_m=4)
    try:
        n = H.levels[0].n
        B, X = np.zeros((n, 8)), np.zeros((n, 8))
        assert lib.GeneoTestAmgVcycle(H.h, 0, ac._dp(B), 8, ac._dp(X), 8, 8) == 1
        assert "wider than the hierarchy" in ac.err_text(lib)
        assert lib.GeneoTestAmgVcycle(H.h, H.nlevels, ac._dp(B), 8, ac._dp(X), 8, 1) == 1
        assert "no such level" in ac.err_text(lib)
        assert lib.GeneoTestAmgVcycle(H.h, 0, ac._dp(B), 1, ac._dp(X), 8, 2) == 1
    finally:
        H.destroy()
    bad = suboff.copy()
    bad[-1] -= 1
    with pytest.raises(AssertionError, match="suboff"):
        ac.Hierarchy(lib, a, bad)
