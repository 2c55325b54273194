#!/usr/bin/env python
"""Measures the flexible CG of KSPSolve_GenEO (-ksp_type fcg).

--kernels: the step x += alpha p, r -= alpha w with |r|^2 on --rows rows, the fused kernel (bk::vec_fcg_step, alpha from the
device) against its composed form (download [eta, pi], bk::axpy, bk::axpy, bk::dot), through GeneoTestKrylovPrimitive: wall
clock around --runs calls, each of which ends in a device synchronise, the best of three such batches; and the same with a
null norm2.  eta is kept at 1 and pi at 1e-9, so that the vectors stay finite over the calls.

--solve: the benchmark's options (-geneo_lvl SRAS,1) on an n^3 grid (default 126), 8 subdomains, one set-up per inner
tolerance.  cg at the benchmark's -dls1_ksp_rtol first, the benchmark's own code path; its true residual |b - A x| / |b| then
is the -ksp_rtol of the fcg runs under -ksp_norm_type unpreconditioned (whose test is the true residual) at -dls1_ksp_rtol
1e-7, 1e-3 and 1e-2: runs that reach the same true residual.  cg at -dls1_ksp_rtol 1e-2, with the benchmark's -ksp_rtol,
stands beside them.  Per run: outer iterations, dls1_iterations, solve seconds, |b - A x| / |b|, the counters.

Each leg is a child process of its own under --leg-timeout seconds; a leg that fails or runs out of time ends the run.  One
JSON document on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels_leg(args):
    from geneo4petsc_amd import _lib
    from geneo4petsc_amd.pc import DeviceVector
    lib = _lib.load()
    n, rng = args.rows, np.random.default_rng(3)

    def call(name, I, P):
        ia = (C.c_int * len(I))(*I)
        da = (C.c_double * 1)(0.0)
        pa = (C.c_void_p * len(P))(*P)
        rc = lib.GeneoTestKrylovPrimitive(name.encode(), ia, da, pa)
        if rc < 0:
            raise RuntimeError("%s: rc %d (%s)" % (name, rc, lib.PCGenEOGetError(None).decode()))
        return rc

    def best(fn):
        fn()
        out = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(args.runs):
                fn()
            out.append((time.perf_counter() - t0) / args.runs)
        return min(out)

    base = rng.standard_normal(n) / np.sqrt(n)
    x, r, p, w = (DeviceVector.from_host(lib, np.roll(base, 17 * i)) for i in range(4))
    S = DeviceVector.from_host(lib, np.array([1.0, 1e-9]))
    n2, work = DeviceVector(lib, 1), DeviceVector(lib, call("vec_dot_nwg", [n], [None]))
    rec = {"rows": n, "calls_per_batch": args.runs}
    for fused in (1, 0, 1, 0):                            # alternating: the second pair shows the spread
        lib.GeneoSetKernelVariant(b"krylov_fused", fused)
        key = "fused" if fused else "composed"
        rec.setdefault("step_norm_" + key + "_ms", []).append(
            1e3 * best(lambda: call("vec_fcg_step", [n], [x.ptr, r.ptr, p.ptr, w.ptr, S.ptr, n2.ptr, work.ptr])))
        rec.setdefault("step_" + key + "_ms", []).append(
            1e3 * best(lambda: call("vec_fcg_step", [n], [x.ptr, r.ptr, p.ptr, w.ptr, S.ptr, None, None])))
    lib.GeneoSetKernelVariant(b"krylov_fused", 1)
    rec["bytes_fused"] = 6 * 8 * n
    rec["bytes_composed"] = 8 * 8 * n
    rec["step_norm_fused_GBps"] = 1e-9 * rec["bytes_fused"] / (1e-3 * min(rec["step_norm_fused_ms"]))
    rec["step_norm_composed_GBps"] = 1e-9 * rec["bytes_composed"] / (1e-3 * min(rec["step_norm_composed_ms"]))
    print(json.dumps(rec, indent=1))


def solve_leg(args):
    from geneo4petsc_amd import decomp
    from geneo4petsc_amd.pc import GenEOPC
    n, parts = args.n, (2, 2, 2)
    doms = [decomp.decompose_grid_domain(n, 3, parts, 2, s, native=True) for s in range(8)]
    npart = decomp.structured_node_partition(n, 3, parts)
    b = np.zeros(n ** 3)
    for d in doms:                                        # b = A (1 .. N), from the rows of the domain that owns each node
        rows = d.a_dir @ (d.l2g.astype(np.float64) + 1.0)
        sel = npart[d.l2g] == d.gid
        b[d.l2g[sel]] = rows[sel]
    nb = float(np.linalg.norm(b))
    doc = {"n": n, "dof": n ** 3, "runs": []}

    def run(label, opts, dls1_rtol="1e-07"):
        """a set-up of its own per run: the local solver reads -dls1_ksp_rtol at the set-up"""
        pc = GenEOPC()
        pc.set_from_options(["-geneo_lvl", "SRAS,1", "-geneo_tau", "0.35", "-geneo_cut", "20", "-els2_eps_tol", "0.001", "-ksp_type", "cg",
                             "-ksp_rtol", "1e-05", "-dls1_ksp_rtol", dls1_rtol, "-dls1_pc_type", "amg", "-els2_pc_type", "amg",
                             "-ksp_initial_guess_nonzero", "0"])
        pc.set_sizes(n ** 3, 8)
        for d in doms:
            pc.add_subdomain(d.gid, d.l2g, d.mult, d.a_neu, d.a_dir)
        pc.setup(b)
        for k, v in opts:
            pc.set_option(k, v)
        best = None
        for _ in range(args.runs):
            i0 = pc.info()["dls1_iterations"]
            x, its, rnorm, reason = pc.solve(b, x0=np.zeros_like(b))
            info = pc.info()
            k = pc.krylov_info()
            rec = dict(label=label, its=its, reason=reason, rnorm=rnorm, dls1_iterations=int(info["dls1_iterations"] - i0),
                       solve_s=info["solveTime"], true_rel=float(np.linalg.norm(b - pc.matmult(x)) / nb),
                       pc_applies=k["pc_applies"], mat_mults=k["mat_mults"], fcg=pc.fcg_info())
            if best is None or rec["solve_s"] < best["solve_s"]:
                best = rec
        best["setup_s"] = pc.info()["setupTime"]
        pc.destroy()
        doc["runs"].append(best)
        return best

    cg = run("cg, -dls1_ksp_rtol 1e-7", [])
    target = repr(cg["true_rel"])
    for tol in ("1e-7", "1e-3", "1e-2"):
        run("fcg unpreconditioned, -dls1_ksp_rtol " + tol,
            [("-ksp_type", "fcg"), ("-ksp_norm_type", "unpreconditioned"), ("-ksp_rtol", target)], tol)
    run("cg, -dls1_ksp_rtol 1e-2", [], "1e-2")
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--n", type=int, default=126)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg-timeout", type=int, default=420)
    ap.add_argument("--leg", choices=["kernels", "solve"], default=None, help="(internal)")
    args = ap.parse_args()
    if args.leg == "kernels":
        return kernels_leg(args)
    if args.leg == "solve":
        return solve_leg(args)
    doc = {}
    for leg in [l for l, on in (("kernels", args.kernels), ("solve", args.solve)) if on]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rows", str(args.rows), "--n", str(args.n), "--runs", str(args.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        if r.returncode:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the %s leg failed with status %d" % (leg, r.returncode))
        doc[leg] = json.loads(r.stdout[r.stdout.index("{"):])
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
