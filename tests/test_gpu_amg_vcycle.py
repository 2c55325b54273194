"""-m gpu: the multigrid hierarchy and its V-cycle on the device against the longdouble reference of amg_cases.py: every
form of the cycle (fused with M, two-launch, without the pre-scaled copy, unfused, Chebyshev degrees 2 and 3, depths 1, 2
and 3; device, host and host-with-uploaded-R set-ups), the set-up against scipy, independence of a subdomain's cycle from
its batch, and the single-precision companions: read at m = 1 when the hierarchy asks for them, never otherwise.
The figures are printed (pytest -s)."""
import numpy as np
import pytest

import amg_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()          # raises if the HIP library is missing: no fallback


@pytest.fixture(scope="module")
def blocks():
    return ac.make_blocks()


@pytest.fixture(scope="module")
def batch(blocks):
    return ac.batch_of(blocks)


@pytest.mark.parametrize("name", list(ac.CYCLE_CASES))
def test_cycle_against_reference(lib, monkeypatch, batch, name):
    a, suboff = batch
    nlev, err, err64, vec_lpr = ac.run_cycle_case(lib, monkeypatch, name, a, suboff, "gpu")
    if nlev >= 3:
        # the coarse Galerkin operators are ragged: their products ran the lanes-per-row kernels
        assert any(v > 0 for v in vec_lpr[1:]), vec_lpr
    assert err <= ac.CYCLE_BOUND


@pytest.mark.parametrize("setup", ["device", "host"])
def test_hierarchy_against_scipy(lib, monkeypatch, batch, setup):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    H = ac.Hierarchy(lib, a, suboff, setup=setup)
    try:
        assert H.nlevels >= 3
        ac.assert_identities(H, a, "gpu/" + setup)
    finally:
        H.destroy()


def test_device_and_host_setups_agree(lib, monkeypatch, batch):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    Hd = ac.Hierarchy(lib, a, suboff, setup="device")
    Hh = ac.Hierarchy(lib, a, suboff, setup="host")
    try:
        ac.assert_same_hierarchy(Hd, Hh, a, "gpu")
    finally:
        Hd.destroy()
        Hh.destroy()


@pytest.mark.parametrize("degree", [1, 2])
def test_cycle_does_not_depend_on_the_batch(lib, monkeypatch, blocks, batch, degree):
    ac.set_env(monkeypatch, {})
    ac.check_batch_independence(lib, blocks, batch, degree, "gpu")


# ---- single-precision companions ------------------------------------------------------------------------------------
def _apply(H, m, ldb, ldx, seed):
    n = H.levels[0].n
    B = np.random.default_rng(seed).standard_normal((n, ldb))
    X = np.full((n, ldx), ac.SENT)
    B0 = B.copy()
    H.vcycle(0, B, X, m)
    assert B.tobytes() == B0.tobytes()
    assert np.all(X[:, m:].view(np.int64) == np.float64(ac.SENT).view(np.int64))
    return B0[:, :m], X[:, :m]


@pytest.mark.parametrize("setup,fine_companion", [("device", False), ("device", True), ("host", False)])
def test_single_hierarchy_reads_companions_at_m1_only(lib, monkeypatch, batch, setup, fine_companion):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    H = ac.Hierarchy(lib, a, suboff, setup=setup, single=True, fine_companion=fine_companion)
    try:
        assert H.lp_matrices > 0
        l0 = H.levels[0]
        # the fine level is a stencil: everything on it is on the sliced path and carries a companion except the
        # ragged restriction
        assert l0.fused and l0.M is not None and l0.Acs is not None
        assert l0.lp["A"] and l0.lp["Acs"] and l0.lp["P"] and l0.lp["M"]
        assert H.lp_matrices == sum(lv.lp[k] for lv in H.levels for k in ac.MATRICES)
        tag = "gpu single/%s%s" % (setup, "+fine-companion" if fine_companion else "")
        # m = 1, contiguous: the float-rounded entries, FP64 arithmetic
        B, X = _apply(H, 1, 1, 1, 501)
        rounded, plain = ac.ref_vcycle(H, 0, B, ac.LD, rounded=True), ac.ref_vcycle(H, 0, B, ac.LD)
        apart = ac.rel_err(rounded, plain)
        err = ac.rel_err(X, rounded)
        print("amg-single %s m=1 err=%.2e against the rounded reference (rounded and unrounded references %.2e apart) bound=%.1e"
              % (tag, err, apart, ac.CYCLE_BOUND))
        assert apart > 1e4 * ac.CYCLE_BOUND          # the two references are told apart by the bound
        assert err <= ac.CYCLE_BOUND
        # blocks, and a single vector on the block path, read FP64
        for m, ldb, ldx, seed in ((16, 19, 96, 502), (1, 1, 3, 503)):
            B, X = _apply(H, m, ldb, ldx, seed)
            err = ac.rel_err(X, ac.ref_vcycle(H, 0, B, ac.LD))
            print("amg-single %s m=%d ldx=%d err=%.2e against the unrounded reference bound=%.1e" % (tag, m, ldx, err, ac.CYCLE_BOUND))
            assert err <= ac.CYCLE_BOUND
    finally:
        H.destroy()


def test_double_hierarchy_ignores_a_borrowed_companion(lib, monkeypatch, batch):
    a, suboff = batch
    ac.set_env(monkeypatch, {})
    H = ac.Hierarchy(lib, a, suboff, setup="device", single=False, fine_companion=True)
    try:
        assert H.lp_matrices == 0
        assert H.levels[0].lp["A"]                     # its owner's companion is there ...
        assert not any(lv.lp[k] for lv in H.levels for k in ("Acs", "P", "R", "M"))
        B, X = _apply(H, 1, 1, 1, 504)
        err = ac.rel_err(X, ac.ref_vcycle(H, 0, B, ac.LD))
        print("amg-single gpu double+fine-companion m=1 err=%.2e against the unrounded reference bound=%.1e" % (err, ac.CYCLE_BOUND))
        assert err <= ac.CYCLE_BOUND                   # ... and the cycle does not read it
    finally:
        H.destroy()
