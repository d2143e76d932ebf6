"""One rank of a multi-rank run of every preconditioner that materialises z -- BJ(4), ISAI, GISAI, IC, ILU, IRILU and
Multigrid, each of the rank's LOCAL block (Preconditioner.H:47-81) -- against the distributed oracle, bit for bit.
Launched by test_gpu_precond_ranks.py through torch.distributed.run (gloo rendezvous on 127.0.0.1); one launch loops over
all its kinds and solvers on one process group and one registry.

With these kinds z comes from launches of its own (krylov_plan's `generic`), step_1x puts p formed from that z and the
merged multi-rank turn stands down: fusedTurnInUse is 0 for every case here.

modes
  oracle    CPU only: every distributed reference solve used by the GPU modes stops by the tolerance before maxIter, after
            at least 10 checks, at the global x*; every Multigrid hierarchy has at least 3 levels.
  gpu-host  the host-buffer transport (callbacks -> gloo).
  gpu-peer  the scalar all-reduces through the peer mesh, summed in rank order."""
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
from helpers import oracle_precond_renumbered, to_new  # noqa: E402
from dist_worker import allreduce, allreduce_rank_order, gather_global, make_exchange, oracle_dist_matrix  # noqa: E402
import precond_cases as pc  # noqa: E402
from test_gpu_multigrid import assert_hierarchy  # noqa: E402

TOL, MAX_ITER = 1e-11, 300   # (the criterion of tests/dist_worker.py)
# (symmetric BJ(4) + GMRES(20) is left out: its reference reaches maxIter without meeting the tolerance)
CASES = {
    "sym": [("BJ4", "cg"), ("ISAI", "cg"), ("GISAI", "cg"), ("IC", "cg"), ("MG", "cg"), ("ISAI", "gmres"), ("MG", "gmres")],
    "asym": [("BJ4", "bicgstab"), ("GISAI", "bicgstab"), ("ILU", "bicgstab"), ("IRILU", "bicgstab"), ("MG", "bicgstab"),
             ("GISAI", "gmres"), ("ILU", "gmres")],
}
DIRECT = {"BJ4": dict(max_block_size=4), "ISAI": dict(isai="spd"), "GISAI": dict(isai="general")}
KIND_IDS = dict(pc.KIND_IDS, BJ4=capi.PRECOND_BJ, ISAI=capi.PRECOND_ISAI, GISAI=capi.PRECOND_GISAI)


def make_case(args, rank, world, symmetric):
    """(this rank's case, the global case)"""
    if args.random >= 0:  # (as dist_worker --random: an irregular global system cut into row blocks of random sizes)
        rng = np.random.default_rng(args.random)
        n_glob = int(rng.integers(600, 2500))
        glob = synthetic.random_global_case(n_glob, int(rng.integers(1, 5)), int(rng.choice([4, 60, 900])),
                                            symmetric=symmetric, seed=args.random)
        cuts = np.sort(rng.choice(np.arange(1, n_glob), world - 1, replace=False))
        return synthetic.partition_rows(glob, [0, *[int(c) for c in cuts], n_glob], rank), glob
    gx, gy, gz = map(int, args.shape.split(","))
    px, py, pz = map(int, args.procs.split(","))
    assert px * py * pz == world
    kw = dict(symmetric=True) if symmetric else dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
    return synthetic.poisson_block(gx, gy, gz, px, py, pz, rank, **kw), synthetic.poisson_block(gx, gy, gz, **kw)


class Block:
    """One rank's share of a system and everything that is the same for all its kinds and solvers."""

    def __init__(self, args, rank, world, symmetric):
        self.case, glob = make_case(args, rank, world, symmetric)
        self.xs_g = synthetic.x_star(glob.global_index, glob.global_n)
        self.b = synthetic.apply_case(glob, self.xs_g)[self.case.global_index]
        self.reduce = allreduce_rank_order if args.mode == "gpu-peer" else allreduce
        self.A, self.csr, self.nl, self.comm = oracle_dist_matrix(self.case, self.reduce)
        self.refs = {}

    def ref(self, kind):
        """The NumPy reference of a callback kind on the local block, in the caller's numbering."""
        if kind not in self.refs:
            self.refs[kind] = pc.make_ref(kind, *self.csr)
        return self.refs[kind]

    def renumbered(self, new_id):
        """The oracle's system in the numbering the library chose for this rank (as dist_worker.run_case)."""
        rp, cols, vals = self.csr
        p_rp, p_cols, p_vals, _ = orc.permute_csr(rp, cols, vals, new_id)
        n_rows, n_cols, n_vals, _ = orc.permute_non_local(self.nl[0], self.nl[1], self.nl[3], new_id)
        ex, comm = make_exchange(None), self.comm
        A = orc.DistMatrix(p_rp, p_cols, p_vals, orc.rowptr_from_rows(self.case.n_cells, n_rows), n_cols, n_vals,
                           new_id[comm[2]].astype(np.int32), n_halo=n_rows.size,
                           exchange=lambda s_: ex(comm[0], comm[1], s_), allreduce=self.reduce,
                           global_n=self.case.global_n)
        return A, (p_rp, p_cols, p_vals)

    def oracle_precond(self, kind, new_id=None, csr=None):
        """(the oracle's preconditioner of the local block, z(r) in the caller's order)"""
        if kind in DIRECT:
            if new_id is None:
                P = orc.Precond(*self.csr, **DIRECT[kind])
                return P, P.apply
            P = oracle_precond_renumbered(orc, self.case, *csr, new_id, **DIRECT[kind])
            return P, lambda r: P.apply(to_new(r, new_id))[new_id]
        return pc.callback(self.ref(kind).apply, new_id), self.ref(kind).apply

    def reference(self, kind, solver, new_id=None):
        A, csr = (self.A, self.csr) if new_id is None else self.renumbered(new_id)
        P, apply = self.oracle_precond(kind, new_id, csr)
        b = self.b if new_id is None else to_new(self.b, new_id)
        ref = pc.oracle_solve(A, b, P, solver, tolerance=TOL, max_iter=MAX_ITER)
        if new_id is not None:
            ref.x = ref.x[new_id]
        return ref, apply


def assert_sound(blk, ref, kind, solver):
    """What a reference must satisfy to pin anything: it stops by the tolerance before maxIter, after at least 10 checks,
    at the solution; a Multigrid hierarchy has at least 3 levels."""
    cap = 2 * MAX_ITER if solver == "bicgstab" else MAX_ITER  # (the criterion counts GKOBiCGStab's half steps)
    assert ref.final_residual <= TOL and 10 <= ref.n_iterations <= cap, (kind, solver, ref.n_iterations, ref.final_residual)
    err = np.abs(ref.x - blk.xs_g[blk.case.global_index]).max()
    assert err <= 1e-6, (kind, solver, err)
    if kind == "MG":
        assert blk.ref(kind).levels >= 3, blk.ref(kind).levels


def check_reference(blk, kind, solver, rank):
    ref, _ = blk.reference(kind, solver)
    assert_sound(blk, ref, kind, solver)
    err = np.abs(gather_global(blk.case, ref.x) - blk.xs_g).max()
    assert err <= 1e-7, (kind, solver, err)
    print(f"rank {rank}: {kind} {solver}: {ref.n_iterations} checks, |x - x*| {err:.1e}", flush=True)


def check_device(args, blk, reg, kind, solver, rank):
    case = blk.case
    cfg = capi.default_config(
        solver=pc.SOLVER_IDS[solver], krylov_dim=pc.KRYLOV_DIM, preconditioner=KIND_IDS[kind],
        max_block_size=4 if kind == "BJ4" else 1, tolerance=TOL, rel_tol=0.0, max_iter=MAX_ITER, export_res=1,
        adapt_min_iter=0, matrix_format=capi.FORMAT_CSR, force_host_buffer=1,
        renumber=capi.RENUMBER_ON if args.renumber else capi.RENUMBER_OFF)
    s = reg.solver(f"{'sym' if case.symmetric else 'asym'}_{kind}_{solver}", cfg)
    s.set_property("peerSafeWait", 0.0)  # (as dist_worker: the fused waits, not the single waiter of ranks sharing a device)
    if kind == "MG":
        s.set_multigrid(**pc.MG_DEFAULTS)
    s.set_matrix(case)
    new_id = s.renumbering()
    assert (new_id is not None) == bool(args.renumber)
    x, perf = s.solve(blk.b, np.zeros_like(blk.b))
    hist = s.history()
    assert s.get_property("fusedTurnInUse") == 0.0  # (a materialised z: the merged multi-rank turn stands down)
    ref, apply = blk.reference(kind, solver, new_id)
    assert_sound(blk, ref, kind, solver)
    # the preconditioner alone: the local block's, in the caller's order
    r = np.random.default_rng(3 + rank).standard_normal(case.n_cells)
    if kind == "MG":
        assert_hierarchy(s, blk.ref(kind))
    np.testing.assert_array_equal(s.apply_preconditioner(r), apply(r), err_msg=f"z of {kind}")
    # the solve: same local trees, same order of the sum over ranks
    assert perf.n_iterations == (ref.n_iterations // 2 if solver == "bicgstab" else ref.n_iterations), (
        kind, solver, perf.n_iterations, ref.n_iterations)
    np.testing.assert_array_equal(hist, ref.history, err_msg=f"history of {kind} {solver}")
    np.testing.assert_array_equal(x, ref.x, err_msg=f"x of {kind} {solver}")
    assert perf.n_norm_evals == ref.n_evals and perf.final_residual == ref.final_residual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["oracle", "gpu-host", "gpu-peer"])
    ap.add_argument("--shape", default="12,12,12")
    ap.add_argument("--procs", default="1,1,2")
    ap.add_argument("--system", default="sym", choices=["sym", "asym", "both"])
    ap.add_argument("--random", type=int, default=-1, help="seed: a random irregular global system in row blocks of random sizes")
    ap.add_argument("--renumber", type=int, default=0, help="1: every rank's device copy in an RCM numbering of its own")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    orc.build()
    reg = None
    if args.mode != "oracle":
        reg = capi.Registry(device_id=rank % max(1, torch.cuda.device_count()))
        ex = make_exchange(None)
        reg.set_host_comm(rank, world, allreduce, lambda nb, ct, s: ex(nb, ct, s))
        if args.mode == "gpu-peer":
            handles = [None] * world
            dist.all_gather_object(handles, reg.peer_handle())
            reg.peer_connect(rank, world, handles)
    for name in (["sym", "asym"] if args.system == "both" else [args.system]):
        blk = Block(args, rank, world, name == "sym")
        if args.random >= 0:  # (what the random cut is for: ranks with unequal numbers of neighbours)
            counts = allreduce(np.eye(world)[rank] * blk.comm[0].size)
            assert len(set(counts.tolist())) > 1, counts
        for kind, solver in CASES[name]:
            if args.mode == "oracle":
                check_reference(blk, kind, solver, rank)
            else:
                check_device(args, blk, reg, kind, solver, rank)
    if reg is not None:
        reg.close()
    dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
