"""Blocks of right-hand sides on two ranks (CPU, gloo, host twin): PCMatApply_GenEO and KSPMatSolve_GenEO at world size 2
equal the one-rank results -- the apply to the parity bound of tests/block_rhs_util.py, the solve with the same counts and
reasons per column --, halo buffers narrower than the block width are a set-up error, and the exchange callback gets the
plain direction flag from the single-vector path and direction | width << 1 from the block path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import block_rhs_util as U
import cases
from test_gloo import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 16
ARGV = ["-geneo_lvl", "ASM,1"] + U.BASE + U.SOLVE


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    """one two-rank run for the tests of this module: (inputs Xa, Bs; the worker's arrays; its meta record)"""
    tmp_path = tmp_path_factory.mktemp("block_gloo")
    mesh, dec, a, b = cases.grid_case(12, 3, (2, 2, 2), 1)
    N = mesh.nbNode
    Xa = U.rhs_block(N, 17, 31)                                     # two slabs, the second padded
    Bs = np.stack([a @ np.ones(N), np.random.default_rng(21).standard_normal(N), np.random.default_rng(26).standard_normal(N),
                   np.zeros(N)], axis=1)
    Bs = np.concatenate([Bs, Bs[:, 1:2]], axis=1)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "res.npz")
    np.savez(inp, Xa=Xa, Bs=Bs)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "block_gloo_worker.py"), out, inp, str(W)] + ARGV
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    return Xa, Bs, got, json.loads(str(got["meta"]))


def test_exchange_flags(two_ranks):
    """A host's callback written for single vectors may compare the flag with 0 and 1: no width bits at width 1."""
    meta = two_ranks[3]
    assert meta["flags_vector"] == [0, 1]
    assert meta["flags_block"] == [0 | W << 1, 1 | W << 1]


def test_two_ranks_equal_one_rank(two_ranks):
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    mesh, dec, a, b = cases.grid_case(12, 3, (2, 2, 2), 1)
    N = mesh.nbNode
    Xa, Bs, got, meta = two_ranks
    assert "-geneo_block_width" in meta["narrow"] and "PCGenEOSetCommWidth" in meta["narrow"], meta["narrow"]
    pc = cases.run_pc(lib, mesh, dec, ARGV + ["-geneo_block_width", str(W)], b)
    Y1 = pc.mat_apply(Xa)
    err = U.relcols(got["Y"], Y1)
    print("PCMatApply, two ranks against one: %.3e (bound %.1e)" % (err, U.PARITY_BOUND))
    assert err <= U.PARITY_BOUND
    # the inputs: no column hovers at its threshold in the one-rank single-vector solves
    for j in range(Bs.shape[1]):
        x, its, rnorm, reason = pc.solve(Bs[:, j], x0=np.zeros(N))
        hist = pc.residual_history()
        if its:
            thr = 1e-10 * hist[0]
            assert hist[-1] < 0.95 * thr and hist[-2] > 1.05 * thr, "bad input: column %d hovers (%.3e, %.3e against %.3e)" % (
                j, hist[-2], hist[-1], thr)
    X1, its1, rnorm1, reasons1 = pc.mat_solve(Bs)
    print("KSPMatSolve, two ranks: its %s, one rank: %s" % (meta["its"], list(its1)))
    assert meta["its"] == [int(v) for v in its1] and meta["reasons"] == list(reasons1)
    assert len(set(meta["its"])) >= 3
    for j in (0, 1, 2, 4):
        assert np.linalg.norm(got["X"][:, j] - X1[:, j]) <= 1e-10 * np.linalg.norm(X1[:, j])
    assert not np.any(got["X"][:, 3]) and np.array_equal(got["X"][:, 4], got["X"][:, 1])
    assert meta["info"]["width"] == W and meta["info"]["padded"] > 0
    pc.destroy()
