"""Flexible CG of KSPSolve_GenEO (-ksp_type fcg) on two ranks (CPU, gloo, host twin): ASM,1 at 12^3 with one and with two
subdomains per rank, under both norm types.  The count and the reason equal the one-rank run's on the same decomposition, and
the history and the solution agree with it to the parity bound of tests/fcg_util.py; the right-hand side is checked first,
on the numpy reference alone, not to hover at its threshold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import fcg_util as F
from test_gloo import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVL, N = "ASM,1", 12
# (parts, norm) -> (seed, -ksp_rtol), picked as the seeds of fcg_util.SEEDS
GLOO_SEEDS = {
    ((2, 1, 1), 'preconditioned'): (1, 8.752e-09),
    ((2, 1, 1), 'unpreconditioned'): (1, 3.473e-09),
    ((2, 2, 1), 'preconditioned'): (1, 1.25e-08),
    ((2, 2, 1), 'unpreconditioned'): (1, 1.874e-10),
}


@pytest.mark.parametrize("norm", ["preconditioned", "unpreconditioned"])
@pytest.mark.parametrize("parts", [(2, 1, 1), (2, 2, 1)])
def test_two_ranks_equal_one_rank(tmp_path, parts, norm):
    from hostsim_util import hostsim_lib
    lib = hostsim_lib()
    seed, rtol = GLOO_SEEDS[(parts, norm)]
    mesh, dec, a, _ = cases.grid_case(n=N, parts=parts, overlap=2)
    b = np.random.default_rng(seed).standard_normal(mesh.nbNode)
    argv = F.argv_for(LVL, F.CHEB) + ["-ksp_type", "fcg", "-ksp_norm_type", norm, "-ksp_rtol", repr(rtol),
                                      "-ksp_initial_guess_nonzero", "0"]
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    xr, its_r, hist_r, reason_r = F.reference_fcg(pc, b, None, 0, norm=norm, rtol=rtol)
    bad = F.input_ok(hist_r, its_r, rtol * hist_r[0])
    assert reason_r == "KSP_CONVERGED_RTOL" and bad is None, "bad input: %s: pick another seed" % bad
    x1, its1, rnorm1, reason1 = pc.solve(b, x0=np.zeros_like(b))
    hist1 = pc.residual_history().copy()
    pc.destroy()
    assert its1 == its_r and reason1 == "KSP_CONVERGED_RTOL"
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "res.npz")
    np.savez(inp, b=b)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "fcg_gloo_worker.py"), out, inp] + \
        [str(p) for p in parts] + argv
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    meta = json.loads(str(got["meta"]))
    err = float(np.linalg.norm(got["x"] - x1) / np.linalg.norm(x1))
    assert meta["subdomains_here"] == parts[0] * parts[1] * parts[2] // 2
    assert meta["its"] == its1 and meta["reason"] == reason1
    dh = float(np.max(np.abs(got["hist"] - hist1)) / hist1[0])
    print("fcg %s, two ranks (%d subdomains each): its %d, one rank %d, hist %.3e (bound %.1e), x %.3e (bound %.1e)" % (
        norm, meta["subdomains_here"], meta["its"], its1, dh, F.PARITY_BOUND["hist"], err, F.PARITY_BOUND["x"]))
    assert dh <= F.PARITY_BOUND["hist"] and err <= F.PARITY_BOUND["x"]
    assert meta["fcg"]["directions"] == min(its1, 31) and meta["fcg"]["steps_composed"] == its1
    assert meta["info"]["pc_applies"] == (its1 + 1 if norm == "preconditioned" else its1) and meta["info"]["basis_vectors"] == 0
