#!/usr/bin/env python
"""Times the coarse operator's factorisation and solve on the device against the host path (-geneo_coarse_device never).

Per size n: the blocked device factorisation and sweeps (GeneoTestCoarseFactor / GeneoTestCoarseSolve, device time between
two events) for every block size asked, and the host code the PC runs without them (the same hooks with nb = 0: host
Cholesky; download, host sweeps, upload -- wall time).  With --pc: the 16^3 / 8 subdomains / tau 0.6 case (dimE = 1256)
set up under `never` and under `auto`, lvl2ApplyEinvTimeLoc and the wall time per apply_q.
With --block, instead: the blocked sweeps on a block of w right-hand sides (GeneoTestCoarseSolveBlock) against w times the
single-vector sweeps (GeneoTestCoarseSolve), device time per sweep pair, for every size, block size and width.
With --block-pc, instead: the same 16^3 case with the Chebyshev local solver and -geneo_block_width 32, PCMatApply on 32
columns -- wall time and lvl2ApplyEinvTimeLoc per slab.  This mode reads nothing a library before the blocked block sweeps
lacks, so the same file times the parent commit from its own tree.  One JSON document on stdout (and in --out)."""
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


def block_hooks(lib, n, blocks, widths, reps, tries):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    a = g @ g.T / n + np.eye(n)
    lo = np.ascontiguousarray(np.linalg.cholesky(0.5 * (a + a.T)))
    lt = np.ascontiguousarray(lo.T)
    B = rng.standard_normal((n, max(widths)))
    rows = []
    for nb in blocks:
        single = []
        for _ in range(tries):
            y = B[:, 0].copy()
            rc = lib.GeneoTestCoarseSolve(n, nb, _p(lo), _p(lt), _p(y), reps)
            if rc:
                raise RuntimeError("solve n=%d nb=%d: rc %d %s" % (n, nb, rc, lib.PCGenEOGetError(None).decode()))
            single.append(elapsed(lib)[1])
        for w in widths:
            blk = []
            for _ in range(tries):
                Y = np.ascontiguousarray(B[:, :w]).copy()
                rc = lib.GeneoTestCoarseSolveBlock(n, nb, w, _p(lo), _p(lt), _p(Y), reps)
                if rc:
                    raise RuntimeError("block solve n=%d nb=%d w=%d: rc %d %s" % (n, nb, w, rc, lib.PCGenEOGetError(None).decode()))
                blk.append(elapsed(lib)[1])
            x = np.linalg.solve(lo @ lt, B[:, :w])
            rows.append({"n": n, "nb": nb, "w": w, "reps": reps, "single_ms": min(single), "w_singles_ms": w * min(single),
                         "block_ms": min(blk), "block_over_single": min(blk) / min(single),
                         "w_singles_over_block": w * min(single) / min(blk),
                         "relative_error": float(np.linalg.norm(Y - x) / np.linalg.norm(x))})
    return rows


def block_pc_case(lib, applies, width=32):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    from geneo4petsc_amd.pc import DeviceVector
    mesh, dec, a, b = cases.grid_case(n=16, parts=(2, 2, 2), overlap=1)
    argv = ["-geneo_lvl", "SRAS,1", "-geneo_tau", "0.6", "-ksp_type", "cg", "-dls1_ksp_type", "chebyshev", "-dls1_ksp_rtol", "1e-7",
            "-geneo_block_width", str(width)]
    pc = cases.run_pc(lib, mesh, dec, argv, b)
    n = mesh.nbNode
    X = np.random.default_rng(5).standard_normal((n, width))
    xd, yd = DeviceVector.from_host(lib, np.asfortranarray(X).ravel(order="F")), DeviceVector(lib, n * width)
    out = {"coarse_info": pc.coarse_info(), "width": width, "applies": applies}

    def timed(label):
        for _ in range(3):
            assert lib.PCMatApply_GenEO(pc.h, xd.ptr, n, yd.ptr, n, width) == 0
        lib.GeneoDeviceSync()
        i0 = pc.info()
        t0 = time.perf_counter()
        for _ in range(applies):
            lib.PCMatApply_GenEO(pc.h, xd.ptr, n, yd.ptr, n, width)
        lib.GeneoDeviceSync()
        wall = (time.perf_counter() - t0) / applies
        i1 = pc.info()
        out[label] = {"mat_apply_wall_ms": 1e3 * wall,
                      "lvl2ApplyEinvTimeLoc_ms_per_slab": 1e3 * (i1["lvl2ApplyEinvTimeLoc"] - i0["lvl2ApplyEinvTimeLoc"]) / applies,
                      "lvl2ApplyZtTimeLoc_ms_per_slab": 1e3 * (i1["lvl2ApplyZtTimeLoc"] - i0["lvl2ApplyZtTimeLoc"]) / applies}

    timed("default")
    if hasattr(pc, "coarse_block_counters"):
        out["counters_default"] = pc.coarse_block_counters()
        lib.GeneoSetKernelVariant(b"block_fused", 0)        # the composed forms, E^-1 column by column
        timed("block_fused_0")
        lib.GeneoSetKernelVariant(b"block_fused", 1)
        out["counters_after_block_fused_0"] = pc.coarse_block_counters()
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
    ap.add_argument("--block", action="store_true", help="the sweeps on blocks against w x the single-vector sweeps")
    ap.add_argument("--widths", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--block-pc", action="store_true", help="PCMatApply on 32 columns at dimE 1256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from geneo4petsc_amd import _lib
    lib = _lib.load()
    if args.block or args.block_pc:
        doc = {}
        if args.block:
            doc["block_hooks"] = [r for n in args.sizes for r in block_hooks(lib, n, args.blocks, args.widths, args.reps, args.tries)]
        if args.block_pc:
            doc["block_pc_dimE_1256"] = block_pc_case(lib, args.applies)
    else:
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
