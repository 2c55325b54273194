#!/usr/bin/env python
"""Measures the right-preconditioned / flexible GMRES of KSPSolve_GenEO (-ksp_pc_side right, -ksp_type fgmres).

--kernels: one Gram-Schmidt step on --rows rows at --nb basis vectors, the fused pair (bk::vec_gs_dots, bk::vec_gs_update
with the norm) against its composed form (nb bk::dot, nb bk::axpy, one bk::dot), through GeneoTestKrylovPrimitive: wall
clock around --runs calls, each of which ends in a device synchronise, the best of three such batches.

--solve: the benchmark's options with -geneo_lvl RAS,1 on an n^3 grid (default 126), 8 subdomains, one set-up.  Left GMRES
at the benchmark's -dls1_ksp_rtol first; its true residual |b - A x| / |b| then is the -ksp_rtol of the flexible runs (whose
test is the true residual) at -dls1_ksp_rtol 1e-7, 1e-3 and 1e-2: runs that reach the same true residual.  Per run: outer
iterations, dls1_iterations, solve seconds, |b - A x| / |b|.

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
    n, nb, rng = args.rows, args.nb, np.random.default_rng(3)

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
    V = [DeviceVector.from_host(lib, np.roll(base, 17 * i)) for i in range(nb)]
    Wd, Yd = DeviceVector.from_host(lib, base), DeviceVector.from_host(lib, base)
    tab = DeviceVector.from_host(lib, np.array([v.ptr for v in V], dtype=np.uint64).view(np.float64))
    Hd, Cd = DeviceVector(lib, nb), DeviceVector.from_host(lib, np.full(nb, 1e-3))
    n2, work = DeviceVector(lib, 1), DeviceVector(lib, call("vec_dot_nwg", [n], [None]) * nb)
    rec = {"rows": n, "nb": nb, "calls_per_batch": args.runs}
    for fused in (1, 0):
        lib.GeneoSetKernelVariant(b"krylov_fused", fused)
        key = "fused" if fused else "composed"
        rec["dots_" + key + "_ms"] = 1e3 * best(lambda: call("vec_gs_dots", [nb, n], [tab.ptr, Wd.ptr, Hd.ptr, work.ptr]))
        rec["update_" + key + "_ms"] = 1e3 * best(lambda: call("vec_gs_update", [nb, n], [Yd.ptr, tab.ptr, Cd.ptr, n2.ptr, work.ptr]))
        rec["step_" + key + "_ms"] = rec["dots_" + key + "_ms"] + rec["update_" + key + "_ms"]
    lib.GeneoSetKernelVariant(b"krylov_fused", 1)
    gb = 8e-9 * n
    rec["dots_fused_GBps"] = gb * (nb + -(-nb // 8)) / (1e-3 * rec["dots_fused_ms"])
    rec["update_fused_GBps"] = gb * (nb + 2) / (1e-3 * rec["update_fused_ms"])
    rec["bytes_fused"] = (2 * nb + -(-nb // 8) + 2) * 8 * n
    rec["bytes_composed"] = (5 * nb + 2) * 8 * n
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
        pc.set_from_options(["-geneo_lvl", "RAS,1", "-geneo_tau", "0.35", "-geneo_cut", "20", "-els2_eps_tol", "0.001", "-ksp_type", "gmres",
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
            rec = dict(label=label, its=its, reason=reason, rnorm=rnorm, dls1_iterations=int(info["dls1_iterations"] - i0),
                       solve_s=info["solveTime"], true_rel=float(np.linalg.norm(b - pc.matmult(x)) / nb), krylov=pc.krylov_info())
            if best is None or rec["solve_s"] < best["solve_s"]:
                best = rec
        best["setup_s"] = pc.info()["setupTime"]
        pc.destroy()
        doc["runs"].append(best)
        return best

    left = run("gmres left, -dls1_ksp_rtol 1e-7", [])
    target = repr(left["true_rel"])
    run("gmres right, -dls1_ksp_rtol 1e-7", [("-ksp_pc_side", "right"), ("-ksp_rtol", target)])
    for tol in ("1e-7", "1e-3", "1e-2"):
        run("fgmres, -dls1_ksp_rtol " + tol, [("-ksp_type", "fgmres"), ("-ksp_rtol", target)], tol)
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--nb", type=int, default=15)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rows", str(args.rows), "--nb", str(args.nb), "--n", str(args.n),
               "--runs", str(args.runs)]
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
