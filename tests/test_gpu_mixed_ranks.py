"""GPU tests of the mixed-precision mode of GKOCG on several ranks (property mixedPrecision; DESIGN.md section 7c, "several
ranks"): the fp32 halo and the all-reduced wide sums on the peer mesh (the waiting finish kernel and the single waiter of
peerSafeWait), the host-buffer rung and the RCCL rung (the stand-in), every rank compared bit for bit with the per-rank walk
of tests/mixed_ranks_walk.py -- x, the exported history, the counts, the stop reason, the distributed fp32 product -- plus
the overflow that ends the solve on every rank by agreement, the double path without the keyword, and a time-step loop whose
ledger stops moving.  Each test is one launch of tests/mixed_ranks_worker.py (at most 3 ranks: 5 processes with the device
open); a launch that fails is not started again.  What the references must satisfy: tests/test_mixed_ranks_walk.py."""
import os
import socket
import subprocess
import sys

import pytest

from mixed_ranks_worker import LAUNCHES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "cpp", "librccl_standin.so")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_launch(name):
    n, args = LAUNCHES[name]
    assert n <= 3
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OGL_PEER_TIMEOUT_S="20")
    if "gpu-rccl" in args:
        if not os.path.exists(STANDIN):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "librccl_standin.so"])
        env["OGL_RCCL_LIBRARY"] = STANDIN
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "mixed_ranks_worker.py"), *args]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    assert p.returncode == 0, (p.stdout[-4000:], p.stderr[-8000:])
    for rank in range(n):
        assert f"rank {rank} ok" in p.stdout
