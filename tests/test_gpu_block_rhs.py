"""-m gpu: blocks of right-hand sides on the device (-geneo_block_width 16 | 32; csrc/block_dev.hip), HIP library, no
fallback: the checks of tests/block_rhs_util.py that the host twin runs too, then what only the GPU has -- the HIP graph of
a slab's local solve with the counters of what ran, the kernels against their composed forms, released memory, and the GPU
against the host twin."""
import ctypes as C

import numpy as np
import pytest

import block_rhs_util as U
from primitive_cases import same_bits

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


def test_options_and_errors(lib):
    U.check_options_and_errors(lib)


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("with_dscale", [False, True])
def test_cheb_dir_block_equals_cheb_dir_column_by_column(lib, w, flags, with_dscale):
    U.check_cheb_dir_block(lib, w, flags, with_dscale)
    if w == 32 and with_dscale:
        with U.block_fused_off(lib):                     # the composed form: same bits
            U.check_cheb_dir_block(lib, w, flags, with_dscale)


@pytest.mark.parametrize("w", [16, 32])
def test_import_export(lib, w):
    U.check_import_export(lib, w)


@pytest.mark.parametrize("w", [16, 32])
def test_coldot(lib, w):
    U.check_coldot(lib, w)


@pytest.mark.parametrize("w", [16, 32])
def test_column_updates(lib, w):
    U.check_col_updates(lib, w)


@pytest.mark.parametrize("w", [16, 32])
@pytest.mark.parametrize("n", [1, 17, 160, 1024])
def test_chol_solve_block(lib, w, n):
    U.check_chol_solve_block(lib, w, n)


@pytest.mark.parametrize("n,w,m", [(20, 32, 33), (12, 16, 5)])
def test_mat_mult(lib, n, w, m):
    U.check_mat_mult(lib, n, w, m)


@pytest.mark.parametrize("n,w", [(20, 32), (12, 16)])
@pytest.mark.parametrize("lvl", U.LEVELS)
@pytest.mark.parametrize("m", [5, 33])
def test_mat_apply_equals_apply(lib, n, w, lvl, m):
    U.check_mat_apply(lib, n, w, lvl, m)


@pytest.mark.parametrize("n,w,lvl", [(20, 32, "SRAS,1"), (12, 16, "ASM,H1")])
def test_column_independence(lib, n, w, lvl):
    U.check_column_independence(lib, n, w, lvl)


def test_symmetry_and_linearity_at_the_default_precision(lib):
    U.check_symmetry(lib, 20, 32)


@pytest.mark.parametrize("w,lvl,seeds", [(16, "ASM,1", (21, 23)), (32, "ASM,1", (21, 23))])
def test_mat_solve_equals_solve_column_by_column(lib, w, lvl, seeds):
    U.check_mat_solve(lib, 12, w, lvl, seeds)


def test_graph_counters_and_composed_forms(lib):
    """3 applies of 33 columns at w = 32: 6 slabs, 99 columns, 93 zero columns of padding, and every local solve but the
    first replayed from the HIP graph -- a silent fall-back to direct launches would show here.  The composed forms
    ("block_fused" 0) give the bits of the kernels."""
    mesh, dec, a, b = U.grid(20)
    import cases
    pc = cases.run_pc(lib, mesh, dec, U.argv_for("SRAS,1", 32, U.DOUBLE), b)
    X = U.rhs_block(mesh.nbNode, 33, 15)
    assert pc.block_info() == dict(width=32, slabs=0, columns=0, padded=0, graph_launches=0)
    Y = [pc.mat_apply(X) for _ in range(3)]
    assert pc.block_info() == dict(width=32, slabs=6, columns=99, padded=93, graph_launches=5)
    assert same_bits(Y[0], Y[1]) and same_bits(Y[0], Y[2])
    with U.block_fused_off(lib):
        Y0 = pc.mat_apply(X)                                 # same PC: the graph is recaptured for the other form
    assert same_bits(Y0, Y[0]), "composed forms: %.3e" % U.relcols(Y0, Y[0])
    pc.destroy()


def test_resetup(lib):
    U.check_resetup(lib)


def test_released_memory():
    """A set-up without a width behind one with width 32 leaves the library's live device bytes (GeneoDeviceMemInfo) where
    a fresh set-up without a width has them, and destroy leaves what the destroy of a PC without a width leaves.  In a process of its own without the
    caching allocator, whose whole-block accounting depends on what earlier work parked (block_rhs_util.memory_readings)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GENEO_ALLOC_CACHE="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "block_mem_worker.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = json.loads([l for l in r.stdout.splitlines() if l.startswith("READINGS ")][-1][9:])
    print(m)
    assert m["with_width"] > m["fresh"] > 0
    assert m["width_removed"] == m["fresh"], m
    # (what outlives a PC are the library's own lazily made scratch blocks, a few KB: the same with and without a width)
    assert m["destroyed"] == m["fresh_destroyed"] < 65536, m


def test_gpu_equals_host_twin(lib, host):
    mesh, dec, a, b = U.grid(12)
    X = U.rhs_block(mesh.nbNode, 33, 16)
    worst = 0.0
    for lvl in U.LEVELS:
        yg = U.get_pc(lib, 12, U.argv_for(lvl, 16, U.DOUBLE)).mat_apply(X)
        yh = U.get_pc(host, 12, U.argv_for(lvl, 16, U.DOUBLE)).mat_apply(X)
        err = U.relcols(yg, yh)
        print("PCMatApply, GPU against host twin, 12^3 %s: %.3e (bound %.1e)" % (lvl, err, U.PARITY_BOUND))
        worst = max(worst, err)
    assert worst <= U.PARITY_BOUND
