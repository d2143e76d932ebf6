"""IC / ILU / IRILU on two ranks (tests/factor_worker.py): the host-buffer transport and the peer mesh.  Two ranks share
the device with the launcher and this process: four processes with the GPU open."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("mode,kind", [("gpu-host", "IC"), ("gpu-peer", "IC"), ("gpu-peer", "ILU"),
                                       ("gpu-host", "IRILU")])
def test_two_ranks(mode, kind):
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "factor_worker.py"), "--mode", mode, "--kind", kind]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count(" ok") == 2, p.stdout
