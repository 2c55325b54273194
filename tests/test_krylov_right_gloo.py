"""Flexible GMRES of KSPSolve_GenEO (-ksp_type fgmres) on two ranks (CPU, gloo, host twin): RAS,1 at 12^3 with one and with
two subdomains per rank.  The count and the reason equal the one-rank run's on the same decomposition and the solution
agrees with it to the parity bound of tests/krylov_right_util.py; the right-hand side is checked first, on the numpy
reference alone, not to hover at its threshold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import krylov_right_util as K
from test_gloo import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVL, N = "RAS,1", 12
# parts -> (seed, -ksp_rtol), picked as the seeds of krylov_right_util.SEEDS
GLOO_SEEDS = {(2, 1, 1): (1, 1.175e-08), (2, 2, 1): (1, 6.36e-09)}


@pytest.mark.parametrize("parts", [(2, 1, 1), (2, 2, 1)])
def test_two_ranks_equal_one_rank(tmp_path, parts):
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    seed, rtol = GLOO_SEEDS[parts]
    mesh, dec, a, _ = cases.grid_case(n=N, parts=parts, overlap=2)
    b = np.random.default_rng(seed).standard_normal(mesh.nbNode)
    argv = K.argv_for(LVL, K.CHEB) + ["-ksp_type", "fgmres", "-ksp_rtol", repr(rtol), "-ksp_initial_guess_nonzero", "0"]
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    xr, its_r, hist_r, _ = K.reference_fgmres(pc, b, None, 30, 0, rtol=rtol)
    bad = K.input_ok(hist_r, its_r, 30, 0, b, rtol)
    assert bad is None, "bad input: %s: pick another seed" % bad
    x1, its1, rnorm1, reason1 = pc.solve(b, x0=np.zeros_like(b))
    pc.destroy()
    assert its1 == its_r and reason1 == "KSP_CONVERGED_RTOL"
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "res.npz")
    np.savez(inp, b=b)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "krylov_right_gloo_worker.py"), out, inp] + \
        [str(p) for p in parts] + argv
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    meta = json.loads(str(got["meta"]))
    err = float(np.linalg.norm(got["x"] - x1) / np.linalg.norm(x1))
    print("fgmres, two ranks (%d subdomains each): its %d, one rank %d, x %.3e (bound %.1e)" % (
        meta["subdomains_here"], meta["its"], its1, err, K.PARITY_BOUND["x"]))
    assert meta["subdomains_here"] == parts[0] * parts[1] * parts[2] // 2
    assert meta["its"] == its1 and meta["reason"] == reason1
    assert err <= K.PARITY_BOUND["x"]
    assert meta["info"]["basis_vectors"] == 2 * its1 + 2 and meta["info"]["pc_applies"] == its1
