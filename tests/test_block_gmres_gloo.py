"""Block GMRES of KSPMatSolve_GenEO on two ranks (CPU, gloo, host twin): RAS,1 at 12^3, w = 16.  The counts and reasons
per column equal the one-rank run's and the solution agrees with it to the parity bound of tests/block_gmres_util.py.  The
worker solves twice: with the all-reduce buffer of the existing block worker, and with one of w doubles, through which the
(k + 1) w Gram-Schmidt coefficients of a step go in pieces -- the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import block_gmres_util as G
import block_rhs_util as U
from test_gloo import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVL, N, W, SEEDS = G.CASES[0]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("block_gmres_gloo")
    Bs = np.asarray(G.solve_columns(N, tuple(SEEDS)))
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "res.npz")
    np.savez(inp, Bs=Bs)
    argv = G.argv_for(LVL, W)
    argv = [a for i, a in enumerate(argv) if a != "-geneo_block_width" and (i == 0 or argv[i - 1] != "-geneo_block_width")]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "block_gmres_gloo_worker.py"), out, inp, str(W)] + argv
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    return Bs, got, json.loads(str(got["meta"]))


def test_two_ranks_equal_one_rank(two_ranks):
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    Bs, got, meta = two_ranks
    argv = G.argv_for(LVL, W)
    G.check_inputs(G.singles_for(lib, N, argv, G.solve_columns(N, tuple(SEEDS))))
    X1, its1, rnorm1, reasons1 = U.get_pc(lib, N, argv).mat_solve(Bs)
    print("block GMRES, two ranks: its %s, one rank: %s" % (meta["its"], list(its1)))
    assert meta["its"] == [int(v) for v in its1] and meta["reasons"] == list(reasons1)
    err = U.relcols(got["X"], X1)
    print("block GMRES, two ranks against one: %.3e (bound %.1e)" % (err, G.PARITY_BOUND))
    assert err <= G.PARITY_BOUND
    assert not np.any(got["X"][:, 3]) and np.array_equal(got["X"][:, 4], got["X"][:, 1])
    assert meta["wide"]["info"]["width"] == W and meta["wide"]["krylov"]["basis_slabs"] == max(meta["its"]) + 1
    U.release_pcs(lib)


def test_chunked_allreduce(two_ranks):
    """an all-reduce buffer of w doubles: more calls, none longer than w, and the bits of the run with the wide buffer"""
    Bs, got, meta = two_ranks
    assert meta["its_s"] == meta["its"] and meta["reasons_s"] == meta["reasons"]
    assert meta["narrow"]["longest"] == W < meta["wide"]["longest"]
    assert meta["narrow"]["calls"] > meta["wide"]["calls"]
    assert np.array_equal(got["Xs"], got["X"]) and np.array_equal(got["rnorm_s"], got["rnorm"])
