"""Blocks of right-hand sides on the host twin (-geneo_block_width 16 | 32): options and errors, the composed forms of the
block primitives alone, MatMatMult / PCMatApply against their single-vector counterparts, column independence, symmetry,
and KSPMatSolve against KSPSolve column by column.  The checks live in tests/block_rhs_util.py and run unchanged on the
GPU (tests/test_gpu_block_rhs.py)."""
import pytest

import block_rhs_util as U


@pytest.fixture(scope="module")
def lib():
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


def test_resetup(lib):
    """a second set-up followed by an apply; and a set-up without a width after one with: the single-vector bits of a PC
    that never had one (the device-memory readings are a GPU test: the host twin keeps no account)"""
    U.check_resetup(lib)
