"""Every preconditioner that materialises z on two and three ranks against the distributed oracle, bit for bit
(tests/precond_ranks_worker.py): per rank the local block's z, the hierarchy of Multigrid, and history, x and the counts of
whole solves.  One launch runs all its kinds and solvers; at most three ranks share the device with the launcher and this
process: five processes with the GPU open.  A launch that fails is not started again."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(n, *args):
    assert n <= 3
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "precond_ranks_worker.py"), *args]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count(" ok") == n, p.stdout


GPU_LAUNCHES = {
    # 864 rows per rank: two chunks, the boundary in the second
    "peer-sym-2": (2, "--mode", "gpu-peer", "--shape", "12,12,12", "--procs", "1,1,2", "--system", "sym"),
    "peer-asym-3": (3, "--mode", "gpu-peer", "--shape", "12,12,12", "--procs", "1,1,3", "--system", "asym"),
    "host-sym-2": (2, "--mode", "gpu-host", "--shape", "12,12,12", "--procs", "1,1,2", "--system", "sym"),
    # 1,642 rows cut at 111 and 940: one, two and one neighbours
    "peer-random-3": (3, "--mode", "gpu-peer", "--random", "31", "--system", "sym"),
    # every rank in an RCM numbering of its own
    "peer-renumbered-2": (2, "--mode", "gpu-peer", "--shape", "10,10,10", "--procs", "1,1,2", "--system", "sym",
                          "--renumber", "1"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_LAUNCHES))
def test_ranks_equal_the_distributed_oracle(name):
    launch(*GPU_LAUNCHES[name])


def test_the_distributed_references_are_sound():
    """CPU only: the references of the launches above stop by the tolerance, after 10 checks or more, at the global x*."""
    launch(3, "--mode", "oracle", "--shape", "12,12,12", "--procs", "1,1,3", "--system", "both")
