"""One rank of a multi-rank run of preconditioner Chebyshev -- the polynomial of the rank's LOCAL block, no halo exchange
inside an apply -- against the distributed oracle with the walk of tests/chebyshev_walk.py called
back on the local rows, bit for bit.  Launched by test_gpu_chebyshev.py through torch.distributed.run (gloo rendezvous on
127.0.0.1); one launch loops over its cases on one process group and one registry.

modes
  oracle    CPU only: every distributed reference solve stops by the tolerance before maxIter at the global x*.
  gpu-host  the host-buffer transport (callbacks -> gloo).
  gpu-peer  the peer mesh: halo puts, the sums all-reduced inside the finalisers in rank order."""
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
from helpers import blocked  # noqa: E402
from dist_worker import allreduce, allreduce_rank_order, gather_global, make_exchange, oracle_dist_matrix  # noqa: E402
import chebyshev_walk as cw  # noqa: E402

TOL, MAX_ITER, KRYLOV_DIM, DEGREE = 1e-9, 300, 10, 3
SOLVERS = {"cg": capi.SOLVER_CG, "gmres": capi.SOLVER_GMRES}
# (solver, chebyshevFused)
CASES = [("cg", 1), ("cg", 0), ("gmres", 1)]
CHUNK = 512  # (ogl_reduction_chunk_rows(): asserted against the library in the gpu modes)


class Block:
    """One rank's share of the 12 x 12 x 12 box cut 1 x 1 x 2 and what all its cases share."""

    def __init__(self, args, rank, world):
        self.rank = rank
        self.case = synthetic.poisson_block(12, 12, 12, 1, 1, world, rank)
        glob = synthetic.poisson_block(12, 12, 12)
        self.xs_g = synthetic.x_star(glob.global_index, glob.global_n)
        self.b = synthetic.apply_case(glob, self.xs_g)[self.case.global_index]
        reduce = allreduce_rank_order if args.mode in ("gpu-peer", "oracle") else allreduce
        self.A, self.csr, _, self.comm = oracle_dist_matrix(self.case, reduce)
        self.walk = cw.Walk(orc, *self.csr, degree=DEGREE)
        self.refs = {}

    def reference(self, solver):
        """Computed once; do not change it."""
        if solver not in self.refs:
            kw = dict(tolerance=TOL, rel_tol=0.0, max_iter=MAX_ITER)
            with blocked(orc, CHUNK):
                if solver == "gmres":
                    ref = orc.gmres(self.A, self.b, np.zeros_like(self.b), self.walk.precond(), krylov_dim=KRYLOV_DIM, **kw)
                else:
                    ref = orc.cg(self.A, self.b, np.zeros_like(self.b), self.walk.precond(), **kw)
            self.refs[solver] = ref
        return self.refs[solver]


def assert_sound(blk, ref, solver):
    assert ref.final_residual <= TOL and 5 <= ref.n_iterations <= MAX_ITER, (solver, ref.n_iterations, ref.final_residual)
    err = np.abs(gather_global(blk.case, ref.x) - blk.xs_g).max()
    assert err <= 1e-6, (solver, err)


def check_device(args, blk, reg, solver, fused):
    case = blk.case
    cfg = capi.default_config(solver=SOLVERS[solver], krylov_dim=KRYLOV_DIM, preconditioner=capi.PRECOND_CHEBYSHEV,
                              tolerance=TOL, rel_tol=0.0, max_iter=MAX_ITER, export_res=1, adapt_min_iter=0,
                              matrix_format=capi.FORMAT_CSR, force_host_buffer=1, renumber=capi.RENUMBER_OFF)
    s = reg.solver(f"cheb_{solver}_{fused}", cfg)
    s.set_property("peerSafeWait", 0.0)  # (as dist_worker: the fused waits, not the single waiter of ranks sharing a device)
    s.set_chebyshev(degree=DEGREE)
    s.set_property("chebyshevFused", float(fused))
    s.set_matrix(case)
    x, perf = s.solve(blk.b, np.zeros_like(blk.b))
    hist = s.history()
    half = s.get_property("symmetricHalf") == 1.0 and s.get_property("symmetricHalfPerChunk") == 0.0
    assert half  # (the block's local matrix is a box: the whole-matrix half storage)
    assert s.get_property("chebyshevFusedInUse") == float(fused)
    assert s.get_property("chebyshevLaunchesPerApply") == (DEGREE + 1 if fused else 2 * DEGREE + 1)
    if args.mode == "gpu-peer":
        assert s.get_property("peerHalo") == 1.0
    assert s.get_property("chebyshevLambdaMaxInUse") == blk.walk.table.lambda_max
    ref = blk.reference(solver)
    assert_sound(blk, ref, solver)
    # the preconditioner alone: the local block's
    r = np.random.default_rng(3 + blk.rank).standard_normal(case.n_cells)
    np.testing.assert_array_equal(s.apply_preconditioner(r), blk.walk.apply(r), err_msg=f"z of {solver} {fused}")
    # the solve: same local trees, same order of the sum over ranks
    assert perf.n_iterations == ref.n_iterations, (solver, fused, perf.n_iterations, ref.n_iterations)
    np.testing.assert_array_equal(hist, ref.history, err_msg=f"history of {solver} {fused}")
    np.testing.assert_array_equal(x, ref.x, err_msg=f"x of {solver} {fused}")
    assert perf.n_norm_evals == ref.n_evals and perf.final_residual == ref.final_residual
    print(f"rank {blk.rank}: {solver} fused {fused}: {perf.n_iterations} checks", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["oracle", "gpu-host", "gpu-peer"])
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world <= 3
    dist.init_process_group("gloo", rank=rank, world_size=world)
    orc.build()
    reg = None
    if args.mode != "oracle":
        assert capi.lib().ogl_reduction_chunk_rows() == CHUNK
        reg = capi.Registry(device_id=rank % max(1, torch.cuda.device_count()))
        ex = make_exchange(None)
        reg.set_host_comm(rank, world, allreduce, lambda nb, ct, s: ex(nb, ct, s))
        if args.mode == "gpu-peer":
            handles = [None] * world
            dist.all_gather_object(handles, reg.peer_handle())
            reg.peer_connect(rank, world, handles)
    blk = Block(args, rank, world)
    for solver, fused in CASES:
        if args.mode == "oracle":
            ref = blk.reference(solver)
            assert_sound(blk, ref, solver)
            print(f"rank {rank}: {solver}: {ref.n_iterations} checks", flush=True)
        else:
            check_device(args, blk, reg, solver, fused)
    if reg is not None:
        reg.close()
    dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
