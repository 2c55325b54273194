#!/usr/bin/env python
"""Times the coarse operator's factorisation and solve on the device against the host path (-geneo_coarse_device never).

Per size n: the blocked device factorisation and sweeps (GeneoTestCoarseFactor / GeneoTestCoarseSolve, device time between
two events) for every block size asked, and the host code the PC runs without them (the same hooks with nb = 0: host
Cholesky; download, host sweeps, upload -- wall time).  With --pc: the 16^3 / 8 subdomains / tau 0.6 case (dimE = 1256)
set up under `never` and under `auto`, lvl2ApplyEinvTimeLoc and the wall time per apply_q.  One JSON document on stdout
(and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def elapsed(lib):
    f, s = C.c_double(0.0), C.c_double(0.0)
    lib.GeneoTestCoarseElapsed(C.byref(f), C.byref(s))
    return f.value, s.value


def hooks(lib, n, blocks, reps, tries):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    a = g @ g.T / n + np.eye(n)
    a = np.ascontiguousarray(0.5 * (a + a.T))
    b = rng.standard_normal(n)
    lo, lt = np.empty((n, n)), np.empty((n, n))
    st = C.c_int(0)
    out = {"n": n, "reps": reps, "factor_ms": {}, "solve_ms": {}}
    for nb in [0] + list(blocks):
        key = "host" if nb == 0 else "nb%d" % nb
        fms, sms = [], []
        for _ in range(tries):
            rc = lib.GeneoTestCoarseFactor(n, nb, _p(a), _p(lo), _p(lt), C.byref(st))
            if rc or st.value:
                raise RuntimeError("factor n=%d nb=%d: rc %d status %d %s" % (n, nb, rc, st.value,
                                                                            lib.PCGenEOGetError(None).decode()))
            fms.append(elapsed(lib)[0])
            y = b.copy()
            rc = lib.GeneoTestCoarseSolve(n, nb, _p(lo), _p(lt), _p(y), reps)
            if rc:
                raise RuntimeError("solve n=%d nb=%d: rc %d %s" % (n, nb, rc, lib.PCGenEOGetError(None).decode()))
            sms.append(elapsed(lib)[1])
        out["factor_ms"][key] = min(fms)
        out["solve_ms"][key] = min(sms)
        out.setdefault("residual", {})[key] = float(np.linalg.norm(a @ y - b) / np.linalg.norm(b))
    return out


def pc_case(lib, applies):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    mesh, dec, a, b = cases.grid_case(n=16, parts=(2, 2, 2), overlap=1)
    argv = ["-geneo_lvl", "ASM,1", "-geneo_tau", "0.6", "-ksp_type", "gmres", "-els2_eps_tol", "1e-10", "-ksp_rtol", "1e-8"]
    out = {}
    from geneo4petsc_amd.pc import DeviceVector
    for mode in ("never", "auto"):
        pc = cases.run_pc(lib, mesh, dec, argv + ["-geneo_coarse_device", mode], b)
        bd = DeviceVector.from_host(lib, b)
        pc.apply_q(bd)
        lib.GeneoDeviceSync()
        e0 = pc.info()["lvl2ApplyEinvTimeLoc"]
        t0 = time.perf_counter()
        for _ in range(applies):
            pc.apply_q(bd)
        lib.GeneoDeviceSync()
        wall = (time.perf_counter() - t0) / applies
        info = pc.info()
        x, its, rnorm, reason = pc.solve(b)
        out[mode] = {"coarse_info": pc.coarse_info(), "lvl2SetupETimeLoc_s": info["lvl2SetupETimeLoc"],
                     "lvl2ApplyEinvTimeLoc_ms_per_apply": 1e3 * (info["lvl2ApplyEinvTimeLoc"] - e0) / applies,
                     "apply_q_wall_ms": 1e3 * wall, "gmres_iterations": its}
        pc.destroy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1256, 2560, 5120])
    ap.add_argument("--blocks", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--tries", type=int, default=3)
    ap.add_argument("--pc", action="store_true")
    ap.add_argument("--applies", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from geneo4petsc_amd import _lib
    lib = _lib.load()
    doc = {"hooks": [hooks(lib, n, args.blocks, args.reps, args.tries) for n in args.sizes]}
    if args.pc:
        doc["pc_dimE_1256"] = pc_case(lib, args.applies)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
