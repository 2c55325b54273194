"""Worker of tests/test_block_gmres_gloo.py: two ranks over gloo on the host twin, four of the eight subdomains each;
KSPMatSolve_GenEO with -ksp_matsolve_type gmres on the owned rows of a block given by the test, once with the all-reduce
buffer of tests/block_gloo_worker.py and once with one of w doubles, so that the (k + 1) w coefficients of a step go
through it in k + 1 pieces."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_path, in_path, w = sys.argv[1], sys.argv[2], int(sys.argv[3])
    argv = sys.argv[4:]
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import hostsim_util as hu
    from geneo4petsc_amd import decomp
    from geneo4petsc_amd.comm import TorchComm, gather_owned
    from geneo4petsc_amd.pc import GenEOPC
    n, ov, parts, nb = 12, 2, (2, 2, 2), 8
    sub_rank = np.arange(nb) * size // nb
    doms = [decomp.decompose_grid_domain(n, 3, parts, ov, s) for s in range(nb) if sub_rank[s] == rank]
    plan = decomp.grid_rank_plan(n, 3, parts, ov, sub_rank, rank, size, doms)
    lib = hu.hostsim_lib()
    Bs = np.load(in_path)["Bs"][plan.owned]

    class CountingComm(TorchComm):
        calls, longest = 0, 0

        def allreduce(self, user, count):
            self.calls += 1
            self.longest = max(self.longest, int(count))
            return super().allreduce(user, count)

    def solve(red_capacity):
        comm = CountingComm(plan, "cpu") if red_capacity is None else CountingComm(plan, "cpu", red_capacity)
        pc = GenEOPC(lib)
        pc.set_from_options(argv + ["-geneo_block_width", str(w)])
        pc.set_sizes(n ** 3, nb)
        comm.attach(pc)
        for d in doms:
            pc.add_subdomain(d.gid, d.l2g, d.mult, d.a_neu, d.a_dir)
        pc.setup(None)
        comm.calls = comm.longest = 0
        X, its, rnorm, reasons = pc.mat_solve(Bs)
        if comm.error is not None:
            raise comm.error
        info, kinfo = pc.block_info(), pc.block_krylov_info()
        pc.destroy()
        return X, its, rnorm, reasons, dict(calls=comm.calls, longest=comm.longest, info=info, krylov=kinfo)

    X, its, rnorm, reasons, rec = solve(None)
    Xs, its_s, rnorm_s, reasons_s, rec_s = solve(w)
    full = lambda A: np.stack([gather_owned(np.ascontiguousarray(A[:, j]), plan, n ** 3) for j in range(A.shape[1])], axis=1)
    Xf, Xsf = full(X), full(Xs)
    if rank == 0:
        np.savez(out_path, X=Xf, Xs=Xsf, rnorm=rnorm, rnorm_s=rnorm_s,
                 meta=json.dumps(dict(its=[int(v) for v in its], reasons=list(reasons), its_s=[int(v) for v in its_s],
                                      reasons_s=list(reasons_s), wide=rec, narrow=rec_s)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
