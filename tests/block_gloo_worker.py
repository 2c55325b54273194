"""Worker of tests/test_block_rhs_gloo.py: two ranks over gloo on the host twin, four of the eight subdomains each;
PCMatApply_GenEO and KSPMatSolve_GenEO on the owned rows of a block given by the test, the set-up error of halo
buffers narrower than the block width, and the flags the exchange callback receives from a single-vector apply and
matmult and from a block apply."""
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
    from geneo4petsc_amd.pc import GenEOError, GenEOPC
    n, ov, parts, nb = 12, 1, (2, 2, 2), 8
    sub_rank = np.arange(nb) * size // nb
    doms = [decomp.decompose_grid_domain(n, 3, parts, ov, s) for s in range(nb) if sub_rank[s] == rank]
    plan = decomp.grid_rank_plan(n, 3, parts, ov, sub_rank, rank, size, doms)
    lib = hu.hostsim_lib()
    data = np.load(in_path)
    Xa, Bs = data["Xa"][plan.owned], data["Bs"][plan.owned]

    class RecordingComm(TorchComm):
        flags = None

        def exchange(self, user, flag):
            if self.flags is not None:
                self.flags.add(int(flag))
            return super().exchange(user, flag)

    def make(width):
        comm = RecordingComm(plan, "cpu")
        pc = GenEOPC(lib)
        pc.set_from_options(argv + ["-geneo_block_width", str(w)])
        pc.set_sizes(n ** 3, nb)
        comm.attach(pc)
        if width is not None:
            pc.set_comm_width(width)
        for d in doms:
            pc.add_subdomain(d.gid, d.l2g, d.mult, d.a_neu, d.a_dir)
        return pc, comm

    narrow, _ = make(w // 2)
    try:
        narrow.setup(None)
        err = ""
    except GenEOError as e:
        err = str(e)
    narrow.destroy()
    pc, comm = make(None)
    pc.setup(None)
    comm.flags = set()
    pc.apply(np.ascontiguousarray(Xa[:, 0]))
    pc.matmult(np.ascontiguousarray(Xa[:, 0]))
    flags_vector, comm.flags = sorted(comm.flags), set()
    Y = pc.mat_apply(Xa)
    flags_block, comm.flags = sorted(comm.flags), None
    X, its, rnorm, reasons = pc.mat_solve(Bs)
    full = lambda A: np.stack([gather_owned(np.ascontiguousarray(A[:, j]), plan, n ** 3) for j in range(A.shape[1])], axis=1)
    Yf, Xf = full(Y), full(X)
    if rank == 0:
        np.savez(out_path, Y=Yf, X=Xf, meta=json.dumps(dict(its=[int(v) for v in its], reasons=list(reasons), narrow=err,
                                                         info=pc.block_info(), flags_vector=flags_vector,
                                                         flags_block=flags_block)))
    if comm.error is not None:
        raise comm.error
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
