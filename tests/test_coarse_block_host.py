"""Blocks of coarse right-hand sides on the host twin (tests/hostsim): a backend without the blocked sweeps on blocks
(coarse_dev.h, bk::coarse_solve_block) answers "not available".  Under -geneo_coarse_device always the twin has neither a
device-made factor nor an uploaded one, so PC::coarse_einv holds the factor on the host: a slab takes one download of its
dimE x w block, the w host solves of the single-vector path, one upload (PCGenEOGetCoarseBlockCounters: host_blocks)."""
import ctypes as C

import numpy as np
import pytest

import block_rhs_util as U
import cases
from primitive_cases import same_bits

ALWAYS = ["-geneo_coarse_device", "always", "-geneo_coarse_block", "16"]


@pytest.fixture(scope="module")
def lib():
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    yield lib
    U.release_pcs(lib)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_hook_answers_not_available(lib):
    n, w = 5, 16
    a = np.eye(n) * 4.0
    y = np.arange(1.0, n * w + 1.0).reshape(n, w)
    y0 = y.copy()
    assert lib.GeneoTestCoarseSolveBlock(n, 16, w, _p(a), _p(a), _p(y), 1) == -3
    assert same_bits(y, y0)


@pytest.mark.parametrize("w", [16, 32])
def test_host_held_factor_takes_one_round_trip_per_slab(lib, w):
    mesh, dec, a, b = U.grid(8)
    pc = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", w, U.DOUBLE + ALWAYS), b)
    dim, on_device, kind, block = pc.coarse_info()
    assert dim > 0 and (on_device, kind, block) == (0, 0, 0)       # no device factor, nothing uploaded
    assert pc.coarse_block_counters() == dict(blocked=0, by_column=0, host_blocks=0)
    X = U.rhs_block(mesh.nbNode, 33, 31)
    Y = pc.mat_apply(X)
    slabs = pc.block_info()["slabs"]
    assert slabs == -(-33 // w)
    assert pc.coarse_block_counters() == dict(blocked=0, by_column=0, host_blocks=slabs)
    ref = np.stack([pc.apply(X[:, j]) for j in range(33)], axis=1)
    err = U.relcols(Y, ref)
    print("PCMatApply against PCApply, host-held factor, w %d: %.3e (bound %.1e)" % (w, err, U.PARITY_BOUND))
    assert err <= U.PARITY_BOUND
    for j in (0, 3, 32):
        yj = pc.mat_apply(X[:, j:j + 1])
        assert same_bits(yj[:, 0], Y[:, j]), "column %d of the block differs from the block of that column alone" % j
    with U.block_fused_off(lib):                          # the variant selects nothing on this path
        assert same_bits(pc.mat_apply(X[:, :5]), Y[:, :5])
    after = pc.coarse_block_counters()
    assert after["blocked"] == after["by_column"] == 0 and after["host_blocks"] == slabs + 4
    pc.setup(b)                                           # a new set-up resets the three
    assert pc.coarse_block_counters() == dict(blocked=0, by_column=0, host_blocks=0)
    pc.destroy()


def test_host_round_trip_has_the_bits_of_the_uploaded_factor(lib):
    """the host sweeps and the twin's chol_solve_block being the same loops, the block with the factor held on the host
    equals the block with the factor uploaded (the default at dimE <= 1024), bit for bit"""
    mesh, dec, a, b = U.grid(8)
    X = U.rhs_block(mesh.nbNode, 5, 32)
    plain = U.get_pc(lib, 8, U.argv_for("SRAS,1", 16, U.DOUBLE))
    assert plain.coarse_info()[2] == 1
    Y = plain.mat_apply(X)
    assert plain.coarse_block_counters() == dict(blocked=0, by_column=0, host_blocks=0)    # chol_solve_block: none of the three
    held = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", 16, U.DOUBLE + ALWAYS), b)
    assert same_bits(held.mat_apply(X), Y)
    held.destroy()


def test_getter_on_a_null_handle(lib):
    v = [C.c_longlong(7) for _ in range(3)]
    assert lib.PCGenEOGetCoarseBlockCounters(None, *[C.byref(x) for x in v]) == -1
    assert [x.value for x in v] == [7, 7, 7]


def test_getter_without_a_width_reports_zeros(lib):
    mesh, dec, a, b = U.grid(8)
    pc = U.get_pc(lib, 8, ["-geneo_lvl", "SRAS,1"] + U.BASE)
    pc.apply(b)
    assert pc.coarse_block_counters() == dict(blocked=0, by_column=0, host_blocks=0)
    assert lib.PCGenEOGetCoarseBlockCounters(pc.h, None, None, None) == 0
