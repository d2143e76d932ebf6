"""One rank of a multi-rank run of the mixed-precision mode of GKOCG (property mixedPrecision; DESIGN.md section 7c,
"several ranks") against the per-rank NumPy walk of tests/mixed_ranks_walk.py, bit for bit.  Launched by
test_mixed_ranks_walk.py and test_gpu_mixed_ranks.py through torch.distributed.run (gloo rendezvous on 127.0.0.1); one launch
loops over its cases on one process group and one registry.

modes
  oracle    CPU only: every walk the GPU launches compare with satisfies what it must to pin anything (assert_sound).
  gpu-host  the host-buffer transport (callbacks -> gloo): halo values widened to doubles, sums through the callback.
  gpu-peer  the peer mesh: 4-byte halo puts, the sums all-reduced inside the finalisers in rank order.
  gpu-rccl  RCCL -- through OGL_RCCL_LIBRARY the stand-in of tests/cpp, which sums in rank order."""
import argparse
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch.distributed as dist  # noqa: E402

from ogl_amd import capi, synthetic  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from helpers import blocked  # noqa: E402
from dist_worker import allreduce, allreduce_rank_order, gather_global, make_exchange, oracle_dist_matrix  # noqa: E402
import mixed_walk as mw  # noqa: E402
from mixed_ranks_walk import RankSystem, mixed_ranks_walk, product32  # noqa: E402

MAX_ITER = 1000
TIGHT, LOOSE = dict(tolerance=1e-10, rel_tol=0.0), dict(tolerance=1e-10, rel_tol=0.01)
# name -> (preconditioner, criterion, inner keywords, config keywords)
SOLVES = {
    "none-tight": ("none", TIGHT, {}, {}),
    "none-loose": ("none", LOOSE, {}, {}),
    "BJ1-tight": ("BJ1", TIGHT, {}, {}),
    "BJ1-loose": ("BJ1", LOOSE, {}, {}),
    "BJ1-tight-csr": ("BJ1", TIGHT, {}, dict(symmetric_half=0, compress_indices=0)),  # (the CSR copy in the loop)
    "imax5": ("none", TIGHT, dict(inner_max_iter=5), {}),  # (the budget path: on RANDOMISED coefficients)
}
# CG restarted every 5 turns stagnates on the Poisson block (sum |r| rises at the third step); on diagonally dominant random
# coefficients it converges, and with this seed the last step, too, runs into the budget: turns [5, 5, 5, 5]
RANDOMISED = {"imax5": 6}
CHUNK = 512  # (ogl_reduction_chunk_rows(): asserted against the library in the gpu modes)

FOUR = "none-tight,none-loose,BJ1-tight,BJ1-loose"
BOX2 = ("--shape", "12,12,12", "--procs", "1,1,2")  # 864 rows per rank: two chunks, the boundary in the second
# The GPU launches of tests/test_gpu_mixed_ranks.py: name -> (ranks, arguments).  tests/test_mixed_ranks_walk.py runs every
# system and case named here in mode oracle.
LAUNCHES = {
    "box2-peer-finish": (2, ("--mode", "gpu-peer", *BOX2, "--peer-safe-wait", "0", "--cases", FOUR + ",overflow")),
    "box2-peer-safe-wait": (2, ("--mode", "gpu-peer", *BOX2, "--cases", FOUR)),
    "box2-host": (2, ("--mode", "gpu-host", *BOX2, "--cases", FOUR + ",overflow")),
    "box2-rccl": (2, ("--mode", "gpu-rccl", *BOX2, "--cases", FOUR)),
    "box2-layouts-budget-plain-steps": (2, ("--mode", "gpu-peer", *BOX2, "--cases", "BJ1-tight-csr,imax5,plain,steps")),
    "box3-two-neighbours": (3, ("--mode", "gpu-peer", "--shape", "12,12,12", "--procs", "1,1,3", "--peer-safe-wait", "0",
                                "--cases", "BJ1-tight,none-loose")),
    "random3": (3, ("--mode", "gpu-peer", "--random", "31", "--cases", "BJ1-tight,none-loose")),
    "renumbered2": (2, ("--mode", "gpu-peer", "--shape", "10,10,10", "--procs", "1,1,2", "--renumber", "1", "--cases",
                        "BJ1-tight,none-loose")),
}


def make_case(args, rank, world):
    """(this rank's case, the global case)"""
    if args.random >= 0:  # (as dist_worker --random: an irregular global system cut into row blocks of random sizes)
        rng = np.random.default_rng(args.random)
        n_glob = int(rng.integers(600, 2500))
        glob = synthetic.random_global_case(n_glob, int(rng.integers(1, 5)), int(rng.choice([4, 60, 900])), symmetric=True,
                                            seed=args.random)
        cuts = np.sort(rng.choice(np.arange(1, n_glob), world - 1, replace=False))
        return synthetic.partition_rows(glob, [0, *[int(c) for c in cuts], n_glob], rank), glob
    gx, gy, gz = map(int, args.shape.split(","))
    px, py, pz = map(int, args.procs.split(","))
    assert px * py * pz == world
    return synthetic.poisson_block(gx, gy, gz, px, py, pz, rank), synthetic.poisson_block(gx, gy, gz)


class Block:
    """One rank's share of the system and what all its cases share: b, the oracle's pieces, the references computed once."""

    def __init__(self, args, rank, world):
        self.rank, self.world = rank, world
        self.case, glob = make_case(args, rank, world)
        self.xs_g = synthetic.x_star(glob.global_index, glob.global_n)
        self.b = synthetic.apply_case(glob, self.xs_g)[self.case.global_index]
        # (the peer mesh and the RCCL stand-in add the ranks' sums in rank order; gloo's order is the host callback's)
        self.reduce = allreduce_rank_order if args.mode in ("gpu-peer", "gpu-rccl", "oracle") else allreduce
        _, self.csr, self.nl, self.comm = oracle_dist_matrix(self.case, self.reduce)
        self.walks = {}

    def system(self, new_id=None):
        """The rank's RankSystem, in the numbering the library chose for it when there is one (as dist_worker.run_case)."""
        rp, cols, vals = self.csr
        nl_rows, nl_cols, nl_vals = self.nl[0], self.nl[1], self.nl[3]
        send = self.comm[2]
        if new_id is not None:
            rp, cols, vals, _ = orc.permute_csr(rp, cols, vals, new_id)
            nl_rows, nl_cols, nl_vals, _ = orc.permute_non_local(nl_rows, nl_cols, nl_vals, new_id)
            send = new_id[send].astype(np.int32)
        ex, ids, sizes = make_exchange(None), self.comm[0], self.comm[1]
        return RankSystem(orc, rp, cols, vals, nl_rows, nl_cols, nl_vals, send, exchange=lambda s: ex(ids, sizes, s),
                          allreduce=self.reduce, global_n=self.case.global_n)

    def walk(self, name, new_id=None, b=None, x0=None, system=None):
        key = (name, None if new_id is None else new_id.tobytes())
        if b is None and key in self.walks:
            return self.walks[key]
        precond, crit, inner, _ = SOLVES[name]
        sysm = system or self.system(new_id)
        to_dev = (lambda v: v) if new_id is None else (lambda v: _to_new(v, new_id))
        bb = self.b if b is None else b
        xx = np.zeros_like(bb) if x0 is None else x0
        inv_d = orc.jacobi_generate_scalar(sysm.rp, sysm.cols, sysm.vals) if precond == "BJ1" else None
        with blocked(orc, CHUNK):
            w = mixed_ranks_walk(sysm, to_dev(bb), to_dev(xx), inv_d, max_iter=MAX_ITER, **crit, **inner)
        if new_id is not None:
            w.x = w.x[new_id]  # back to the caller's order
        if b is None:
            self.walks[key] = w
        return w


def randomise(case, seed):
    """Coefficients that are not representable in binary32, different on every face (the interfaces keep theirs)."""
    rng = np.random.default_rng(seed)
    case.upper[:] = rng.uniform(-1.0, -0.25, case.upper.size)
    case.diag[:] = rng.uniform(7.0, 9.0, case.n_cells)
    return case


def variant(blk, name):
    """The block a case runs on: the launch's own, or its copy with randomised coefficients and b = A x* (collective)."""
    if name not in RANDOMISED:
        return blk
    v = copy.copy(blk)
    v.case = randomise(copy.deepcopy(blk.case), 100 * RANDOMISED[name] + blk.rank)
    _, v.csr, v.nl, v.comm = oracle_dist_matrix(v.case, blk.reduce)
    v.walks = {}
    v.b = v.system().A.apply(blk.xs_g[v.case.global_index])
    return v


def _to_new(v, new_id):
    out = np.empty_like(v)
    out[new_id] = v
    return out


def assert_sound(blk, name, w):
    """What a walk must satisfy to pin anything: it stops on the criterion before maxIter, takes at least 2 outer steps
    under the tight criterion and exactly 1 under relTol 0.01, ends at the global x* (the tight criterion; relTol 0.01 asks
    for two digits of the residual only), meets no subnormal fp32 value on any rank, and every rank counts the same turns."""
    _, crit, inner, _ = SOLVES[name]
    assert w.stop_reason == mw.STOP_CRITERION and w.inner_turns < MAX_ITER, (name, w.stop_reason, w.inner_turns)
    if crit["rel_tol"] > 0:
        assert w.outer_steps == 1, (name, w.outer_steps)
    else:
        assert w.outer_steps >= 2, (name, w.outer_steps)
        err = np.abs(gather_global(blk.case, w.x) - blk.xs_g).max()
        assert err <= 1e-6, (name, err)
    assert w.smallest_fp32 >= mw.TINY32, (name, w.smallest_fp32)
    turns = np.zeros((blk.world, 64))
    turns[blk.rank, :len(w.step_turns)] = w.step_turns
    turns = allreduce(turns.ravel()).reshape(blk.world, 64)
    assert (turns == turns[0]).all(), (name, turns[:, :len(w.step_turns)])
    if "inner_max_iter" in inner:  # (the budget path: every step runs into innerMaxIter)
        assert all(t == inner["inner_max_iter"] for t in w.step_turns), (name, w.step_turns)


def config(args, name, **extra):
    precond, crit, _, ckw = SOLVES[name]
    kw = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ if precond == "BJ1" else capi.PRECOND_NONE,
              max_block_size=1, max_iter=MAX_ITER, export_res=1, adapt_min_iter=0,
              force_host_buffer=int(args.mode != "gpu-rccl"),
              renumber=capi.RENUMBER_ON if args.renumber else capi.RENUMBER_OFF, **crit)
    kw.update(ckw)
    kw.update(extra)
    return capi.default_config(**kw)


def new_solver(args, reg, field, name, **extra):
    s = reg.solver(field, config(args, name, **extra))
    if args.peer_safe_wait >= 0:  # (-1: the library decides -- peer_connect finds ranks that share a device by itself)
        s.set_property("peerSafeWait", float(args.peer_safe_wait))
    return s


def assert_transport(args, s, case):
    on_mesh = args.mode == "gpu-peer"
    assert s.get_property("mixedHaloBytes") == (4.0 if on_mesh else 8.0), s.get_property("mixedHaloBytes")
    if on_mesh and case.n_cells:
        assert s.get_property("peerHalo") == 1.0
        assert s.get_property("peerSafeWaitInUse") == (0.0 if args.peer_safe_wait == 0 else 1.0)


def assert_solve_is_walk(s, x, perf, w, what):
    got = dict(n_iterations=perf.n_iterations, n_evals=perf.n_norm_evals, outer=s.get_property("mixedOuterSteps"),
               turns=s.get_property("mixedInnerTurns"), reason=s.get_property("mixedStopReason"))
    want = dict(n_iterations=w.n_iterations, n_evals=w.n_evals, outer=w.outer_steps, turns=w.inner_turns, reason=w.stop_reason)
    assert s.get_property("mixedPrecisionInUse") == 1.0
    assert got == want, (what, got, want, w.step_turns)
    np.testing.assert_array_equal(s.history(), w.history, err_msg=f"history of {what}")
    np.testing.assert_array_equal(x, w.x, err_msg=f"x of {what}")
    assert perf.initial_residual == w.initial_residual and perf.final_residual == w.final_residual, what


def check_solve(args, blk, reg, name):
    blk = variant(blk, name)
    case = blk.case
    s = new_solver(args, reg, "mx_" + name, name)
    s.set_mixed_precision(True, inner_max_iter=SOLVES[name][2].get("inner_max_iter"))
    s.set_matrix(case)
    new_id = s.renumbering()
    assert (new_id is not None) == bool(args.renumber)
    # the distributed fp32 product alone (collective), in the caller's order
    sysm = blk.system(new_id)
    x32 = np.random.default_rng(5 + blk.rank).uniform(-1, 1, case.n_cells).astype(np.float32)
    y = s.spmv_f32(x32)
    in_dev = x32 if new_id is None else _to_new(x32, new_id)
    ref = product32(sysm, sysm.vals.astype(np.float32), sysm.nl_vals.astype(np.float32), in_dev)
    np.testing.assert_array_equal(y, ref if new_id is None else ref[new_id], err_msg=f"spmv_f32 of {name}")
    layout = s.get_property("mixedInnerLayout")
    if args.renumber or "csr" in name:
        assert layout == 0.0, layout
    elif args.random < 0:
        assert layout == 2.0, layout  # (the structured block: the half storage in the loop)
    x, perf = s.solve(blk.b, np.zeros_like(blk.b))
    w = blk.walk(name, new_id, system=sysm)
    assert_sound(blk, name, w)
    assert_transport(args, s, case)
    assert_solve_is_walk(s, x, perf, w, name)
    assert perf.n_global_rows == case.global_n, (perf.n_global_rows, case.global_n)
    print(f"rank {blk.rank}: {name}: outer {w.outer_steps} turns {w.step_turns} layout {layout} "
          f"haloBytes {s.get_property('mixedHaloBytes')}", flush=True)


def check_overflow(args, blk, reg):
    """One diagonal coefficient of rank 1 beyond binary32: every rank fails at the first outer check, by agreement."""
    case, name, row = blk.case, "BJ1-tight", 77
    s = new_solver(args, reg, "mx_overflow", name)
    s.set_mixed_precision(True)
    good = case.diag[row]
    if blk.rank == 1:
        case.diag[row] = 1e39
    s.set_matrix(case)
    for attempt in range(2):  # (the second solve finds the same copy and must report again)
        t0 = time.time()
        try:
            s.solve(blk.b, np.zeros_like(blk.b))
            raise AssertionError("the solve did not fail")
        except capi.OglError as e:
            took = time.time() - t0
            assert e.status == capi.ERR_INVALID, (e.status, str(e))
            assert ("row %d" % row if blk.rank == 1 else "another rank") in str(e), str(e)
            assert took < 10.0, took  # (OGL_PEER_TIMEOUT_S is 20: nobody waited for a rank that had left)
    case.diag[row] = good
    s.set_matrix(case)
    x, perf = s.solve(blk.b, np.zeros_like(blk.b))
    assert_solve_is_walk(s, x, perf, blk.walk(name), "restored after the overflow")
    print(f"rank {blk.rank}: overflow ok", flush=True)


def check_plain(args, blk, reg):
    """Without the keyword: the double path as before, against the distributed oracle."""
    case, name = blk.case, "BJ1-tight"
    s = new_solver(args, reg, "mx_plain", name)
    s.set_matrix(case)
    x, perf = s.solve(blk.b, np.zeros_like(blk.b))
    assert s.get_property("mixedPrecisionInUse") == 0.0
    sysm = blk.system()
    with blocked(orc, CHUNK):
        ref = orc.cg(sysm.A, blk.b, np.zeros_like(blk.b), orc.jacobi_generate_scalar(*blk.csr), max_iter=MAX_ITER, **TIGHT)
    assert perf.n_iterations == ref.n_iterations
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)
    print(f"rank {blk.rank}: plain ok", flush=True)


def check_steps(args, blk, reg):
    """A time-step loop of four steps: new coefficients every step, the ledger does not move after the second."""
    name = "BJ1-tight"
    s = new_solver(args, reg, "mx_steps", name)
    s.set_mixed_precision(True)
    marks, x = {}, np.zeros(blk.case.n_cells)
    for step in range(4):
        case = randomise(blk.case, 40 + 10 * step + blk.rank)
        b = np.random.default_rng(50 + 10 * step + blk.rank).uniform(-1, 1, case.n_cells)
        s.set_matrix(case)
        _, blk.csr, blk.nl, blk.comm = oracle_dist_matrix(case, blk.reduce)
        w = blk.walk(name, b=b, x0=x)
        x, perf = s.solve(b, x)
        assert w.smallest_fp32 >= mw.TINY32 and w.outer_steps >= 2, (w.smallest_fp32, w.outer_steps)
        assert_solve_is_walk(s, x, perf, w, f"step {step}")
        marks[step] = capi.memory_ledger().as_dict()
    for k in ("device_alloc_calls", "pinned_alloc_calls", "device_bytes", "pinned_bytes"):
        assert marks[3][k] == marks[1][k], (k, marks)
    print(f"rank {blk.rank}: steps ok", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["oracle", "gpu-host", "gpu-peer", "gpu-rccl"])
    ap.add_argument("--shape", default="12,12,12")
    ap.add_argument("--procs", default="1,1,2")
    ap.add_argument("--random", type=int, default=-1, help="seed: a random irregular global system in row blocks of random sizes")
    ap.add_argument("--renumber", type=int, default=0, help="1: every rank's device copy in a numbering of its own")
    ap.add_argument("--peer-safe-wait", type=int, default=-1,
                    help="-1: left to the library (ranks that share a device: on); 0: the waiting finish kernel")
    ap.add_argument("--cases", default="none-tight,none-loose,BJ1-tight,BJ1-loose",
                    help="names of SOLVES, and overflow | plain | steps")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    orc.build()
    reg = None
    if args.mode != "oracle":
        assert capi.lib().ogl_reduction_chunk_rows() == CHUNK
        reg = capi.Registry(device_id=0)  # (every rank on one device: the library finds that out and switches peerSafeWait on)
        if args.mode == "gpu-rccl":
            uid = [capi.rccl_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            reg.init_rccl(rank, world, uid[0])
        else:
            ex = make_exchange(None)
            reg.set_host_comm(rank, world, allreduce, lambda nb, ct, s: ex(nb, ct, s))
            if args.mode == "gpu-peer":
                handles = [None] * world
                dist.all_gather_object(handles, reg.peer_handle())
                reg.peer_connect(rank, world, handles)
    blk = Block(args, rank, world)
    counts = allreduce(np.eye(world)[rank] * blk.comm[0].size)
    if args.random >= 0:  # (what the random cut is for: ranks with unequal numbers of neighbours)
        assert len(set(counts.tolist())) > 1, counts
    elif world == 3:
        assert counts.tolist() == [1.0, 2.0, 1.0], counts  # (the middle rank has two neighbours)
    for name in args.cases.split(","):
        if args.mode == "oracle":
            if name in SOLVES:
                v = variant(blk, name)
                w = v.walk(name)
                assert_sound(v, name, w)
                print(f"rank {rank}: {name}: outer {w.outer_steps} turns {w.step_turns} smallest {w.smallest_fp32:.2e}", flush=True)
        elif name == "overflow":
            check_overflow(args, blk, reg)
        elif name == "plain":
            check_plain(args, blk, reg)
        elif name == "steps":
            check_steps(args, blk, reg)
        else:
            check_solve(args, blk, reg, name)
    if reg is not None:
        reg.close()
    dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
