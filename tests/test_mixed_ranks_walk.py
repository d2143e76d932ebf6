"""CPU tests of the contract of the mixed-precision mode on several ranks (tests/mixed_ranks_walk.py):
on one rank the distributed walk is tests/mixed_walk.py bit for bit, and with 2 and 3 gloo ranks every reference the GPU
launches of tests/test_gpu_mixed_ranks.py compare with satisfies what it must to pin anything (mixed_ranks_worker.assert_sound:
the criterion before maxIter, at least 2 outer steps under the tight criterion and exactly 1 under relTol 0.01, the global x*,
no subnormal fp32 intermediate on any rank, the same turns per step on all ranks)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import blocked, oracle_csr
import mixed_walk as mw
from mixed_ranks_walk import RankSystem, mixed_ranks_walk
from mixed_ranks_worker import LAUNCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape, bj", [((10, 9, 7), True), ((6, 6, 6), False)], ids=["10x9x7-BJ1", "6x6x6-none"])
def test_one_rank_is_the_single_rank_walk(oracle, shape, bj):
    case = synthetic.poisson_block(*shape)
    b = synthetic.rhs_for_x_star(case)[0]
    rp, cols, vals = oracle_csr(oracle, case)
    inv_d = oracle.jacobi_generate_scalar(rp, cols, vals) if bj else None
    kw = dict(tolerance=1e-10, rel_tol=0.0)
    with blocked(oracle, 512):
        one = mw.mixed_walk(oracle, rp, cols, vals, b, np.zeros_like(b), inv_d, **kw)
        got = mixed_ranks_walk(RankSystem(oracle, rp, cols, vals), b, np.zeros_like(b), inv_d, **kw)
    assert one.outer_steps >= 2
    np.testing.assert_array_equal(got.x, one.x)
    np.testing.assert_array_equal(got.history, one.history)
    assert got.step_turns == one.step_turns
    for k in ("n_iterations", "n_evals", "outer_steps", "inner_turns", "stop_reason", "initial_residual", "final_residual",
              "norm_factor", "smallest_fp32"):
        assert getattr(got, k) == getattr(one, k), k


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _systems():
    """(ranks, system arguments) -> the cases any GPU launch runs on it."""
    out = {}
    for n, args in LAUNCHES.values():
        args = list(args)
        system = tuple(a for k in ("--shape", "--procs", "--random") if k in args for a in (k, args[args.index(k) + 1]))
        names = [c for c in args[args.index("--cases") + 1].split(",") if c not in ("plain", "steps")]
        names = ["BJ1-tight" if c == "overflow" else c for c in names]  # (the solve after the coefficient is restored)
        have = out.setdefault((n, system), [])
        have.extend(c for c in names if c not in have)
    return out


SYSTEMS = _systems()


@pytest.mark.parametrize("key", sorted(SYSTEMS), ids=lambda k: "%d-%s" % (k[0], "-".join(k[1][1::2]).replace(",", "x")))
def test_every_reference_of_the_gpu_launches_is_sound(key):
    n, system = key
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "mixed_ranks_worker.py"), "--mode", "oracle",
           *system, "--cases", ",".join(SYSTEMS[key])]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-6000:])
    assert p.stdout.count("ok") >= n
