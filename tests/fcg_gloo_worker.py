"""Worker of tests/test_fcg_gloo.py: two ranks over gloo on the host twin, half of the subdomains each; KSPSolve_GenEO with
-ksp_type fcg on the owned rows of a right-hand side given by the test, from a zero guess."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_path, in_path, px, py, pz = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    argv = sys.argv[6:]
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import hostsim_util as hu
    from geneo4petsc_amd import decomp
    from geneo4petsc_amd.comm import TorchComm, gather_owned
    from geneo4petsc_amd.pc import GenEOPC
    n, ov, parts = 12, 2, (px, py, pz)
    nb = px * py * pz
    sub_rank = np.arange(nb) * size // nb
    doms = [decomp.decompose_grid_domain(n, 3, parts, ov, s) for s in range(nb) if sub_rank[s] == rank]
    plan = decomp.grid_rank_plan(n, 3, parts, ov, sub_rank, rank, size, doms)
    lib = hu.hostsim_lib()
    b = np.load(in_path)["b"][plan.owned]
    comm = TorchComm(plan, "cpu")
    pc = GenEOPC(lib)
    pc.set_from_options(argv)
    pc.set_sizes(n ** 3, nb)
    comm.attach(pc)
    for d in doms:
        pc.add_subdomain(d.gid, d.l2g, d.mult, d.a_neu, d.a_dir)
    pc.setup(None)
    x, its, rnorm, reason = pc.solve(b, x0=np.zeros_like(b))
    if comm.error is not None:
        raise comm.error
    hist, info, fcg = pc.residual_history().copy(), pc.krylov_info(), pc.fcg_info()
    pc.destroy()
    xf = gather_owned(np.ascontiguousarray(x), plan, n ** 3)
    if rank == 0:
        np.savez(out_path, x=xf, hist=hist, meta=json.dumps(dict(its=int(its), reason=reason, rnorm=float(rnorm), info=info,
                                                                fcg=fcg, subdomains_here=len(doms))))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
