"""One rank of a two-rank run of the incomplete factorisations (launched by test_gpu_incomplete_factor_ranks.py through
torch.distributed.run, gloo rendezvous on 127.0.0.1).  The factor is that of the rank's LOCAL block (the non-overlapping
Schwarz wrap, Preconditioner.H:47-81): every rank's z equals the in-file reference of its block, the distributed solve
converges, and a breakdown on one rank fails the solve on every rank.

modes: gpu-host (host-buffer transport: callbacks -> gloo), gpu-peer (scalar all-reduces through the peer mesh)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from ogl_amd import capi, synthetic  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from helpers import oracle_csr  # noqa: E402
from dist_worker import allreduce, make_exchange  # noqa: E402
from test_gpu_incomplete_factor import Ref, rhs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True)
    ap.add_argument("--kind", default="IC")
    args = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    kinds = {"IC": capi.PRECOND_IC, "ILU": capi.PRECOND_ILU, "IRILU": capi.PRECOND_IRILU}
    reg = capi.Registry(device_id=rank % max(1, torch.cuda.device_count()))
    ex = make_exchange(None)
    reg.set_host_comm(rank, world, allreduce, lambda nb, ct, s: ex(nb, ct, s))
    if args.mode == "gpu-peer":
        handles = [None] * world
        dist.all_gather_object(handles, reg.peer_handle())
        reg.peer_connect(rank, world, handles)
    solver = capi.SOLVER_CG if args.kind == "IC" else capi.SOLVER_BICGSTAB
    cfg = capi.default_config(solver=solver, preconditioner=kinds[args.kind], tolerance=1e-9, rel_tol=0.0,
                              max_iter=1000, force_host_buffer=1, renumber=capi.RENUMBER_OFF)
    orc.build()

    # 1. per-rank z = M^-1 r of the local block, and a converging solve
    case = synthetic.poisson_block(12, 12, 12, 1, 1, world, rank=rank, symmetric=args.kind == "IC")
    b, xs = synthetic.rhs_for_x_star(case)
    s = reg.solver("p", cfg).set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    assert perf.final_residual <= 1e-9 and 0 < perf.n_iterations < 1000, (perf.n_iterations, perf.final_residual)
    assert np.abs(x - xs).max() < 1e-5, np.abs(x - xs).max()
    r = rhs(case.n_cells, seed=rank)
    np.testing.assert_array_equal(s.apply_preconditioner(r), Ref(*oracle_csr(orc, case), args.kind, True).apply(r))

    # 2. rank 1's block with a zero pivot (ILU) / a negative diagonal (IC): every rank's solve fails
    bad = synthetic.poisson_block(12, 12, 12, 1, 1, world, rank=rank, symmetric=args.kind == "IC")
    if rank == 1:
        bad.diag = bad.diag.copy()
        bad.diag[0] = -bad.diag[0] if args.kind == "IC" else 0.0
    s2 = reg.solver("bad", capi.default_config(solver=solver, preconditioner=kinds[args.kind], tolerance=1e-9,
                                               rel_tol=0.0, max_iter=50, force_host_buffer=1,
                                               renumber=capi.RENUMBER_OFF)).set_matrix(bad)
    try:
        s2.solve(np.ones(bad.n_cells), np.zeros(bad.n_cells))
        raise AssertionError(f"rank {rank}: the solve with a broken-down factor returned")
    except capi.OglError as e:
        assert e.status == capi.ERR_INVALID and args.kind in str(e), e
        assert ("row 0" in str(e)) if rank == 1 else ("another rank" in str(e)), e
    assert s2.get_property("iluBreakdownRow") == (0.0 if rank == 1 else -1.0)
    reg.close()
    dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
