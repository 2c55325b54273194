#!/usr/bin/env python
"""Times KSPMatSolve_GenEO (-geneo_block_width 32 and 16) against consecutive KSPSolve_GenEO calls on the same right-hand
sides, in one process: the bench options plus -dls1_ksp_type chebyshev on an n^3 grid (default 126), 8 subdomains.

Per width: seconds per column (best and all of --runs runs, wall clock around work that ends in a device synchronise), the
iteration counts, and the device memory the block work space adds (live bytes of a set-up with the width minus those of a
set-up without).  The single-vector leg solves the same columns one after the other on the same set-up, zero initial
guess.  Every width is one GPU step: a child process of its own under --leg-timeout seconds, inside which the block leg and
the single-vector leg share one set-up; a step that fails or runs out of time ends the run, and nothing more is started on
the device.  One JSON document on stdout (and in --out).

--ksp gmres --lvl RAS,1 times the block GMRES (-ksp_matsolve_type gmres) against consecutive KSPSolve_GenEO GMRES calls, for
the non-symmetric modes; the document then also holds the bytes of the Krylov basis (PCGenEOGetBlockKrylovInfo).
--kernels times the two Gram-Schmidt passes of the block GMRES alone (bk::block_gs_dots, bk::block_gs_update with norms)
against their composed forms -- one block_coldot / block_axpy_cols per basis slab -- on a slab of --rows rows at --nb basis
slabs, in one child process under --leg-timeout."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def live_bytes(lib):
    v = C.c_double(0.0)
    lib.GeneoDeviceMemInfo(C.byref(v), None, None, None, None, None, 0)
    return v.value


def kernels_leg(args):
    """the two Gram-Schmidt passes against their composed forms, through GeneoTestBlockPrimitive: wall clock around `runs`
    calls, each of which ends in a device synchronise; the best of three such batches"""
    from geneo4petsc_amd import _lib
    from geneo4petsc_amd.pc import DeviceVector
    lib = _lib.load()
    n, rng = args.rows, np.random.default_rng(3)
    doc = {"rows": n, "calls_per_batch": args.runs, "cases": []}

    def call(name, I, P):
        ia = (C.c_int * len(I))(*I)
        da = (C.c_double * 1)(0.0)
        pa = (C.c_void_p * len(P))(*P)
        rc = lib.GeneoTestBlockPrimitive(name.encode(), ia, da, pa)
        if rc != 1:
            raise RuntimeError("%s: rc %d (%s)" % (name, rc, lib.PCGenEOGetError(None).decode()))

    def best(fn):
        fn()
        out = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(args.runs):
                fn()
            out.append((time.perf_counter() - t0) / args.runs)
        return min(out)

    for w in args.widths:
        nbmax = max(args.nb)
        slab = rng.standard_normal(n * w) / np.sqrt(n)
        V = [DeviceVector.from_host(lib, np.roll(slab, 17 * i)) for i in range(nbmax)]
        Wd, Yd = DeviceVector.from_host(lib, slab), DeviceVector.from_host(lib, slab)
        tab = DeviceVector.from_host(lib, np.array([v.ptr for v in V], dtype=np.uint64).view(np.float64))
        Hd, Cd = DeviceVector(lib, nbmax * w), DeviceVector.from_host(lib, np.full(nbmax * w, 1e-3))
        n2, work = DeviceVector(lib, w), DeviceVector(lib, 1024 * nbmax * w)
        for nb in args.nb:
            rec = {"w": w, "nb": nb}
            for fused in (1, 0):
                lib.GeneoSetKernelVariant(b"block_fused", fused)
                key = "fused" if fused else "composed"
                rec["dots_" + key + "_ms"] = 1e3 * best(lambda: call("block_gs_dots", [nb, n, w], [tab.ptr, Wd.ptr, Hd.ptr, work.ptr]))
                rec["update_" + key + "_ms"] = 1e3 * best(lambda: call("block_gs_update", [nb, n, w], [Yd.ptr, tab.ptr, Cd.ptr, n2.ptr, work.ptr]))
            lib.GeneoSetKernelVariant(b"block_fused", 1)
            slab_gb = 8e-9 * n * w
            rec["dots_fused_GBps"] = slab_gb * (nb + -(-nb // 8)) / (1e-3 * rec["dots_fused_ms"])
            rec["update_fused_GBps"] = slab_gb * (nb + 2) / (1e-3 * rec["update_fused_ms"])
            doc["cases"].append(rec)
    print(json.dumps(doc, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=126)
    ap.add_argument("--rhs", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="*", default=[32, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds one width may take")
    ap.add_argument("--ksp", choices=["cg", "gmres"], default="cg", help="Krylov method of both legs")
    ap.add_argument("--lvl", default=None, help="-geneo_lvl of the set-up (default: the bench option set's SRAS,1)")
    ap.add_argument("--kernels", action="store_true", help="time the Gram-Schmidt passes alone instead")
    ap.add_argument("--rows", type=int, default=2000000, help="--kernels: rows of the slab")
    ap.add_argument("--nb", type=int, nargs="*", default=[15, 31], help="--kernels: basis slabs")
    ap.add_argument("--kernels-leg", action="store_true", help="(internal)")
    ap.add_argument("--leg", type=int, default=0, help="(internal) run this width in this process and print its JSON")
    args = ap.parse_args()
    if args.kernels_leg:
        return kernels_leg(args)
    if args.kernels:
        cmd = [sys.executable, os.path.abspath(__file__), "--kernels-leg", "--rows", str(args.rows), "--runs", str(args.runs),
               "--widths"] + [str(w) for w in args.widths] + ["--nb"] + [str(v) for v in args.nb]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        if r.returncode:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the kernel timing failed with status %d" % r.returncode)
        text = r.stdout[r.stdout.index("{"):]
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text)
        return
    if not args.leg:
        doc = None
        for w in args.widths:
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--rhs", str(args.rhs), "--runs", str(args.runs),
                   "--ksp", args.ksp, "--leg", str(w)] + (["--lvl", args.lvl] if args.lvl else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)      # raises when it runs out
            if r.returncode:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("width %d failed with status %d: nothing more is started" % (w, r.returncode))
            leg = json.loads(r.stdout[r.stdout.index("{"):])
            if doc is None:
                doc = leg
            else:
                doc["widths"].update(leg["widths"])
        text = json.dumps(doc, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    args.widths = [args.leg]
    args.out = None
    import cases
    from geneo4petsc_amd import _lib
    from geneo4petsc_amd.pc import DeviceVector
    lib = _lib.load()
    mesh, dec, a, b = cases.grid_case(n=args.n, parts=(2, 2, 2), overlap=cases.BENCH_OVERLAP)
    N, m = mesh.nbNode, args.rhs
    argv = cases.bench_argv(["-dls1_ksp_type", "chebyshev", "-ksp_initial_guess_nonzero", "0"])
    if args.lvl:
        argv += ["-geneo_lvl", args.lvl]
    if args.ksp == "gmres":
        argv += ["-ksp_type", "gmres", "-ksp_matsolve_type", "gmres"]
    rng = np.random.default_rng(7)
    B = np.empty((N, m))
    B[:, 0] = b
    for j in range(1, m):
        B[:, j] = a @ rng.standard_normal(N)
    doc = {"n": args.n, "rows": N, "rhs": m, "ksp": args.ksp, "argv": argv, "widths": {}}
    pc0 = cases.run_pc(lib, mesh, dec, argv, b)
    base = live_bytes(lib)
    pc0.destroy()
    Bd = DeviceVector.from_host(lib, B.ravel(order="F"))
    for w in args.widths:
        pc = cases.run_pc(lib, mesh, dec, argv + ["-geneo_block_width", str(w)], b)
        added = live_bytes(lib) - base
        Xd = DeviceVector(lib, N * m)
        its, rs, rn = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

        def block():
            rc = lib.KSPMatSolve_GenEO(pc.h, Bd.ptr, N, Xd.ptr, N, m, its.ctypes.data_as(ip), rn.ctypes.data_as(dp), rs.ctypes.data_as(ip))
            if rc:
                raise RuntimeError(lib.PCGenEOGetError(pc.h).decode())
            lib.GeneoDeviceSync()

        sits = np.zeros(m, dtype=np.int32)
        xd = DeviceVector(lib, N)

        def single():
            i1, r1, n1 = C.c_int(0), C.c_int(0), C.c_double(0.0)
            for j in range(m):
                lib.GeneoTestAxpby(xd.ptr, xd.ptr, 0.0, 0.0, N)          # x = 0
                rc = lib.KSPSolve_GenEO(pc.h, Bd.ptr + 8 * j * N, xd.ptr, C.byref(i1), C.byref(n1), C.byref(r1))
                if rc:
                    raise RuntimeError(lib.PCGenEOGetError(pc.h).decode())
                sits[j] = i1.value
            lib.GeneoDeviceSync()

        block()          # warm-up of both legs: first launches, graph captures
        single()
        tb, ts = [], []
        for _ in range(args.runs):          # alternating
            t0 = time.perf_counter(); block(); tb.append((time.perf_counter() - t0) / m)
            t0 = time.perf_counter(); single(); ts.append((time.perf_counter() - t0) / m)
        X = Xd.to_host().reshape((N, m), order="F")
        res = float(np.max(np.linalg.norm(B - a @ X, axis=0) / np.linalg.norm(B, axis=0)))
        doc["widths"][str(w)] = {"block_s_per_column": tb, "single_s_per_column": ts, "block_best": min(tb), "single_best": min(ts),
                                 "ratio_single_over_block": min(ts) / min(tb), "block_iterations": [int(v) for v in its],
                                 "single_iterations": [int(v) for v in sits], "block_reasons": [int(v) for v in rs],
                                 "work_space_bytes": added, "worst_true_residual": res, "block_info": pc.block_info()}
        if args.ksp == "gmres":
            doc["widths"][str(w)]["block_krylov_info"] = pc.block_krylov_info()
        pc.destroy()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
