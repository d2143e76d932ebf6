"""One rank of a two-rank run of IC with triangularSolves isai and factorSweeps (launched by test_gpu_factor_isai.py through
torch.distributed.run, gloo rendezvous on 127.0.0.1; host-buffer transport): 12 x 12 x 12 cut 1,1,2.  The factor and its
approximate inverses are those of the rank's LOCAL block: every rank's z equals the walk (tests/factor_isai_walk.py) on its
block, and the CG history is bit-equal to the distributed oracle with the walk called back per rank."""
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
from dist_worker import allreduce, make_exchange, oracle_dist_matrix  # noqa: E402
import factor_isai_walk as fw  # noqa: E402
import precond_cases as pc  # noqa: E402

TOL, MAX_ITER = 1e-11, 300   # (the criterion of tests/dist_worker.py)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    orc.build()
    reg = capi.Registry(device_id=rank % max(1, torch.cuda.device_count()))
    ex = make_exchange(None)
    reg.set_host_comm(rank, world, allreduce, lambda nb, ct, s: ex(nb, ct, s))
    case = synthetic.poisson_block(12, 12, 12, 1, 1, world, rank)
    glob = synthetic.poisson_block(12, 12, 12)
    xs_g = synthetic.x_star(glob.global_index, glob.global_n)
    b = synthetic.apply_case(glob, xs_g)[case.global_index]
    A, csr, _, _ = oracle_dist_matrix(case, allreduce)
    r = np.random.default_rng(3 + rank).standard_normal(case.n_cells)
    for power, sweeps in ((1, 0), (2, 3)):
        cfg = capi.default_config(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_IC, sparsity_power=power, tolerance=TOL,
                                  rel_tol=0.0, max_iter=MAX_ITER, export_res=1, adapt_min_iter=0, update_init_guess=1,
                                  matrix_format=capi.FORMAT_CSR, force_host_buffer=1, renumber=capi.RENUMBER_OFF)
        s = reg.solver("p", cfg).set_triangular_solves("isai").set_factor_sweeps(sweeps)
        s.set_property("peerSafeWait", 0.0)
        s.set_matrix(case)
        x, perf = s.solve(b, np.zeros_like(b))
        hist = s.history()
        w = fw.Walk(orc, *csr, "IC", power=power, sweeps=sweeps)
        np.testing.assert_array_equal(s.apply_preconditioner(r), w.apply(r), err_msg=f"z, p {power} sweeps {sweeps}")
        assert s.get_property("triangularSolvesInUse") == 1.0 and s.get_property("factorSweepsInUse") == sweeps
        ref = pc.oracle_solve(A, b, pc.callback(w.apply), "cg", tolerance=TOL, max_iter=MAX_ITER)
        assert ref.final_residual <= TOL and 10 <= ref.n_iterations <= MAX_ITER, (ref.n_iterations, ref.final_residual)
        assert np.abs(ref.x - xs_g[case.global_index]).max() <= 1e-6
        np.testing.assert_array_equal(hist, ref.history, err_msg=f"history, p {power} sweeps {sweeps}")
        np.testing.assert_array_equal(x, ref.x)
        assert perf.n_iterations == ref.n_iterations and perf.n_norm_evals == ref.n_evals
        assert perf.final_residual == ref.final_residual
    reg.close()
    dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
