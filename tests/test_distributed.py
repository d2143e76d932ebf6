"""The sharded path (rows split across ranks, halo exchange + scalar all-reduces), world_size 2-8 (2-4 on the GPU).

CPU (`not gpu`): gloo ranks run the ORACLE's distributed CG against the single-rank oracle on the
assembled global system and check the product's host-side pattern per rank.
GPU (`gpu`): two ranks share the one MI355X of a gpurun box and drive libogl_amd through the
host-buffer transport (the reference's forceHostBuffer mode); RCCL is exercised at world_size 1
(RCCL refuses two ranks on one device) -- the multi-GPU RCCL run itself is the driver's scaling bench.
"""
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


# Several ranks on ONE device (what every multi-rank GPU test on a 1-GPU box is; not a deployment -- one rank per device)
# plus this pytest process, which holds a GPU context of its own, plus torch.distributed.run (its launch configuration asks
# torch.cuda.is_available(), which opens the device): at most six processes may have a shared device open at once, so a
# GPU run has at most four ranks.  (Eight ranks on one device also starved each other's first kernels past the peer
# mesh's start-up self-test; a run that fails is not started again.)
MAX_GPU_RANKS = 4


def run_ranks(n, *args, timeout=600, extra_env=None):
    if "oracle" not in args:
        assert n <= MAX_GPU_RANKS, f"{n} GPU ranks: at most {MAX_GPU_RANKS} (+ launcher + this process) may share the device"
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_worker.py"), *args]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count(" ok") == n, p.stdout
    return p.stdout


@pytest.mark.parametrize("shape,procs,n", [("8,8,8", "1,1,2", 2), ("8,6,4", "2,1,1", 2),
                                          ("6,6,6", "1,2,1", 2)])
@pytest.mark.parametrize("precond", [0, 1])
def test_oracle_two_ranks(shape, procs, n, precond):
    run_ranks(n, "--mode", "oracle", "--shape", shape, "--procs", procs, "--precond", str(precond))


def test_oracle_eight_ranks_2x2x2():
    # corner cells own three processor faces: several non-local entries share a row
    run_ranks(8, "--mode", "oracle", "--shape", "8,8,8", "--procs", "2,2,2")


def test_oracle_two_ranks_bicgstab():
    run_ranks(2, "--mode", "oracle", "--shape", "8,8,8", "--procs", "1,1,2", "--asym", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,procs,n", [("16,16,16", "1,1,2", 2), ("12,12,12", "2,2,1", 4)])
@pytest.mark.parametrize("precond", [0, 1])
def test_gpu_host_buffer_transport(shape, procs, n, precond):
    run_ranks(n, "--mode", "gpu-host", "--shape", shape, "--procs", procs, "--precond",
              str(precond))


@pytest.mark.gpu
def test_gpu_host_buffer_transport_bicgstab():
    run_ranks(2, "--mode", "gpu-host", "--shape", "12,12,12", "--procs", "1,1,2", "--asym", "1")


@pytest.mark.gpu
def test_gpu_host_buffer_transport_gmres():
    run_ranks(2, "--mode", "gpu-host", "--shape", "10,10,10", "--procs", "1,1,2", "--gmres", "20")


def test_oracle_two_ranks_gmres():
    run_ranks(2, "--mode", "oracle", "--shape", "8,8,8", "--procs", "1,1,2", "--gmres", "20")


@pytest.mark.gpu
def test_gpu_rccl_single_rank():
    run_ranks(1, "--mode", "gpu-rccl", "--shape", "12,12,12", "--procs", "1,1,1")


# Peer-write all-reduce (PeerArgs, kernels.hpp): the scalar reductions go through hipIpc-mapped
# mailboxes inside the finaliser kernels.  The ranks share the one GPU of the box here (IPC between
# processes on one device); bit-identical to the distributed oracle with rank-ordered sums.
@pytest.mark.gpu
@pytest.mark.parametrize("shape,procs,n", [("16,16,16", "1,1,2", 2), ("12,12,12", "2,2,1", 4),
                                          ("12,12,16", "1,1,4", 4)])
def test_gpu_peer_allreduce_cg(shape, procs, n):
    run_ranks(n, "--mode", "gpu-peer", "--shape", shape, "--procs", procs)


@pytest.mark.gpu
def test_gpu_peer_allreduce_bicgstab():
    run_ranks(3, "--mode", "gpu-peer", "--shape", "12,12,12", "--procs", "1,1,3", "--asym", "1")


@pytest.mark.gpu
def test_gpu_peer_allreduce_gmres():
    run_ranks(2, "--mode", "gpu-peer", "--shape", "10,10,10", "--procs", "1,1,2", "--gmres", "20")


@pytest.mark.gpu
def test_gpu_peer_rank_dropout_fails_loudly():
    # OGL_PEER_TIMEOUT_S shortens the 60 s after which a missing rank ends the solve with ERR_COMM
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OGL_PEER_TIMEOUT_S="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "peer_dropout_worker.py")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count("dropout ok") == 2 and "failed loudly" in p.stdout, p.stdout


# Irregular decompositions: a random global system cut into contiguous row blocks of random sizes
# (rows with several non-local entries, ranks with 1..n-1 neighbours, interfaces of any length).
@pytest.mark.parametrize("seed,n", [(1, 2), (2, 3), (3, 4), (4, 5)])
def test_oracle_random_partition(seed, n):
    run_ranks(n, "--mode", "oracle", "--random", str(seed))


def test_oracle_random_partition_bicgstab():
    run_ranks(3, "--mode", "oracle", "--random", "11", "--asym", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n", [(5, 2), (6, 3), (7, 4), (8, 4)])
def test_gpu_peer_random_partition(seed, n):
    run_ranks(n, "--mode", "gpu-peer", "--random", str(seed))


@pytest.mark.gpu
def test_gpu_peer_random_partition_bicgstab_and_gmres():
    run_ranks(3, "--mode", "gpu-peer", "--random", "9", "--asym", "1")
    run_ranks(3, "--mode", "gpu-peer", "--random", "10", "--gmres", "15")


@pytest.mark.gpu
def test_gpu_host_buffer_random_partition():
    run_ranks(3, "--mode", "gpu-host", "--random", "12")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,extra", [("gpu-peer", []), ("gpu-host", []), ("gpu-peer", ["--asym", "1"]),
                                        ("gpu-peer", ["--gmres", "20"])])
def test_gpu_renumbered_ranks(mode, extra):
    # every rank keeps its device copy in its own RCM numbering; halo columns and the order of the
    # send list are untouched, so the neighbours never notice
    run_ranks(3, "--mode", mode, "--random", "13", "--renumber", "1", *extra)
    run_ranks(2, "--mode", mode, "--shape", "10,10,10", "--procs", "1,1,2", "--renumber", "1", *extra)


def _n_devices():
    import torch
    return torch.cuda.device_count()          # counting does not initialise the GPU


# One rank per DEVICE where the box has two or more: the first place RCCL with two ranks, cross-device IPC stores and
# the spin-wait kernels meet real xGMI links.  On a box with one device the same runs go with the
# ranks sharing it (dist_worker.py puts rank r on device r % devices); RCCL, which refuses two ranks on one device, is
# then the stand-in below (tests/cpp/rccl_standin.cpp).
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gpu-rccl", "gpu-peer", "gpu-host"])
def test_two_devices_one_rank_each(mode):
    n_dev = _n_devices()
    n = min(max(n_dev, 2), MAX_GPU_RANKS)
    env = None
    if mode == "gpu-rccl" and n_dev < 2:
        if not os.path.exists(STANDIN):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "librccl_standin.so"])
        env = {"OGL_RCCL_LIBRARY": STANDIN}
    run_ranks(2, "--mode", mode, "--shape", "16,16,16", "--procs", "1,1,2", extra_env=env)
    run_ranks(n, "--mode", mode, "--random", str(20 + n), extra_env=env)
    if mode == "gpu-peer":
        run_ranks(2, "--mode", mode, "--shape", "12,12,12", "--procs", "1,1,2", "--asym", "1")
        run_ranks(2, "--mode", mode, "--shape", "12,12,12", "--procs", "1,1,2", "--renumber", "1")


@pytest.mark.gpu
def test_gpu_peer_mesh_soak():
    # 40 solves with changing solver / stop position / right-hand side on one persistent set of fields
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "peer_stress_worker.py"), "--solves", "40", "--seed", "21"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count("solves ok") == 3, p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["gpu-host", "gpu-peer"])
def test_gpu_rebuild_forced_by_one_rank(mode):
    # only the last rank's addressing changes between two solves: the rebuild is agreed by all ranks, and
    # the ranks whose own addressing is unchanged must upload their coefficients again
    run_ranks(2, "--mode", mode, "--shape", "10,10,12", "--procs", "1,1,2", "--relabel", "1")
    run_ranks(3, "--mode", mode, "--random", "14", "--relabel", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--asym", "1"], ["--gmres", "20"], ["--renumber", "1"]],
                         ids=["cg", "bicgstab", "gmres", "cg_renumbered"])
def test_gpu_peer_separate_halo_kernels(extra):
    # property haloFused 0: pack + put + signal and wait + non-local + partials as kernels of their own (the
    # default folds the first into step_1x and the second into the local SpMV kernel); same bits either way
    run_ranks(3, "--mode", "gpu-peer", "--random", "15", "--halo-fused", "0", *extra)
    run_ranks(2, "--mode", "gpu-peer", "--shape", "10,10,10", "--procs", "1,1,2", "--halo-fused", "0", *extra)


# The merged multi-rank GKOCG turn: step_1x inside the half-storage SpMV kernel, the neighbours'
# step_2r puts z of their send rows, every rank keeps the old p of its halo columns and forms p_new there itself --
# 4 launches per turn, bit-equal to the 5-launch turn (p put by step_1x) and to the distributed oracle.
@pytest.mark.gpu
@pytest.mark.parametrize("shape,procs,n,precond,both", [("16,16,16", "1,1,2", 2, 1, True), ("12,12,12", "2,2,1", 4, 0, True),
                                                        ("33,17,12", "1,1,3", 3, 1, False), ("20,20,40", "1,2,2", 4, 1, False)])
def test_gpu_peer_merged_turn(shape, procs, n, precond, both):
    run_ranks(n, "--mode", "gpu-peer", "--shape", shape, "--procs", procs, "--precond", str(precond),
              "--expect-merged", "1")
    if both:
        run_ranks(n, "--mode", "gpu-peer", "--shape", shape, "--procs", procs, "--precond", str(precond),
                  "--fused-turn-multi", "0", "--expect-merged", "0")


@pytest.mark.gpu
def test_gpu_peer_merged_turn_stands_down():
    # host-buffer transport / separate halo kernels: all ranks run the 5-launch turn -- what the neighbours put must
    # be the same on every rank (an irregular share on ONE rank: test_gpu_peer_merged_turn_relabel's second solve)
    run_ranks(2, "--mode", "gpu-host", "--shape", "16,16,16", "--procs", "1,1,2", "--expect-merged", "0")
    run_ranks(2, "--mode", "gpu-peer", "--shape", "16,16,16", "--procs", "1,1,2", "--halo-fused", "0",
              "--expect-merged", "0")


@pytest.mark.gpu
def test_gpu_peer_merged_turn_relabel():
    # a rebuild one rank forces between two solves: the second solve's first z put starts from a fresh pattern
    run_ranks(2, "--mode", "gpu-peer", "--shape", "10,10,12", "--procs", "1,1,2", "--relabel", "1")


# 2 ranks x 2.1 M rows (the largest multi-rank oracle comparison was 16^3), 20 turns, both turns
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
def test_gpu_peer_two_ranks_2m_rows_each(fused):
    run_ranks(2, "--mode", "gpu-peer", "--shape", "128,128,256", "--procs", "1,1,2", "--max-iter", "20",
              "--fused-turn-multi", str(fused), "--expect-merged", str(fused), timeout=900)


# BASELINE.json configs[3] and configs[4] at full size (VERDICT r3 "configs_untested") in their 4-WAY form (the cut
# bench.py --config uses at four ranks: 1 x 2 x 2), the four ranks sharing the one device of the box: nothing of the
# assembled 20 M / 50 M-cell system is built (--no-global), every rank compares its matrix blocks, its distributed SpMV
# and its history / iterate bit for bit with the distributed oracle.
# Through the HOST-BUFFER transport: a cut across y puts boundary rows into every chunk, so with the peer mesh every
# workgroup of every rank's SpMV waits for puts -- ranks on ONE device then hold its workgroup slots and can starve each
# other's put kernels until one times out (OGL_ERR_COMM).  With a device per rank the waiting
# workgroups of a rank occupy only its own device; on a shared one the peer mesh is for slab cuts (the tests above,
# profiles/r04_ranks_216.txt) or runs with the single waiter (below).
@pytest.mark.gpu
def test_gpu_config3_four_way_20m_cells():
    # channel-like box of 272^3 = 20.1 M cells cut 1 x 2 x 2: 272 x 136 x 136 = 5.0 M cells and two processor patches per rank
    run_ranks(4, "--mode", "gpu-host", "--shape", "272,272,272", "--procs", "1,2,2", "--precond", "1",
              "--max-iter", "10", "--no-global", "1", timeout=1500)


@pytest.mark.gpu
def test_gpu_config4_four_way_50m_cells_gmres():
    # 368^3 = 49.8 M cells cut 1 x 2 x 2: 12.5 M cells per rank, every rank's cells shuffled in windows of 65536 (an
    # unstructured numbering; the library renumbers its device copy), GKOGMRES(30) + BJ
    run_ranks(4, "--mode", "gpu-host", "--shape", "368,368,368", "--procs", "1,2,2", "--precond", "1", "--gmres", "30",
              "--max-iter", "10", "--no-global", "1", "--shuffle", "65536", "--renumber", "1", timeout=1800)


@pytest.mark.gpu
def test_gpu_config3_four_way_20m_cells_peer_mesh_single_waiter():
    # the same 4 x 5.0 M cells through the PEER MESH (puts into the neighbours' receive blocks, mailbox all-reduces) with
    # property peerSafeWait: one workgroup per rank waits for the flags instead of every boundary workgroup of the SpMV, so
    # ranks on one device cannot starve each other -- two neighbours and 73,984 halo values per rank at full size
    run_ranks(4, "--mode", "gpu-peer", "--shape", "272,272,272", "--procs", "1,2,2", "--precond", "1",
              "--max-iter", "10", "--no-global", "1", "--peer-safe-wait", "1", "--expect-merged", "0", timeout=1500)
    run_ranks(3, "--mode", "gpu-peer", "--random", "15", "--peer-safe-wait", "1", "--asym", "1")


@pytest.mark.gpu
def test_gpu_peer_ranks_sharing_a_device_are_found_and_get_the_single_waiter():
    """peer_connect gathers the ranks' PCI bus ids through the mesh's all-reduce; when two ranks sit on
    one device the single waiter is switched on without the property -- the 1 x 2 x 2 cut of 192^3 (boundary rows in every
    chunk) passes bit-equal to the distributed oracle as it is."""
    if _n_devices() >= 4:
        pytest.skip("a device per rank: nothing is shared")
    run_ranks(4, "--mode", "gpu-peer", "--shape", "192,192,192", "--procs", "1,2,2", "--max-iter", "5", "--no-global", "1",
              "--peer-safe-wait", "-1", "--expect-merged", "0", timeout=900)


# ---- the RCCL rung with MORE THAN ONE RANK, on one GPU: a stand-in for librccl ----
# Real RCCL refuses two ranks on one device, and the pool has 1-GPU boxes: until a node with a device per rank runs the
# driver's scaling bench, the transport the OpenFOAM hook uses by default (ogl_amd/foam/GKOSolvers.C:76-105) would have
# executed at world_size 1 only.  tests/cpp/rccl_standin.cpp provides the ten entry points comm.cpp binds (shared memory
# between the rank processes, stream-synchronous, all-reduce in rank order); through OGL_RCCL_LIBRARY it takes librccl's
# place, and everything ABOVE the library call runs as it will on a node: ncclCommInitRank + the collective self-test, the
# grouped ncclSend / ncclRecv of every halo exchange on the communication stream with its two events, the ncclAllReduce
# between the reduce- and the logic-finaliser, the agreement on pattern rebuilds -- for slabs, 2 x 2 x 2 cuts, random
# partitions with 1 .. n-1 neighbours per rank, all three solvers; every rank bit-identical to the distributed oracle.
# Reference: DevicePersistent/ExecutorHandler/ExecutorHandler.H:140-144,167-172, CsrMatrixWrapper.H:195-204.
STANDIN = os.path.join(ROOT, "tests", "cpp", "librccl_standin.so")


def rccl_standin_ranks(n, *args, **kw):
    if not os.path.exists(STANDIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "librccl_standin.so"])
    return run_ranks(n, "--mode", "gpu-rccl", *args, extra_env={"OGL_RCCL_LIBRARY": STANDIN}, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,procs,n", [("16,16,16", "1,1,2", 2), ("12,12,12", "2,2,1", 4), ("12,12,12", "1,1,3", 3),
                                          ("12,12,16", "1,1,4", 4)])
@pytest.mark.parametrize("precond", [0, 1])
def test_gpu_rccl_rung_several_ranks(shape, procs, n, precond):
    rccl_standin_ranks(n, "--shape", shape, "--procs", procs, "--precond", str(precond))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n", [(21, 2), (22, 3), (23, 4), (24, 4)])
def test_gpu_rccl_rung_random_partition(seed, n):
    # ranks with 1 .. n-1 neighbours, interfaces of any length: asymmetric neighbour lists inside one ncclGroup
    # (not more ranks than this: every collective of the stand-in is a host round trip of EVERY rank, and seven processes
    #  time-sliced on one GPU took 10-15 s per collective in places -- slowness of the oversubscribed box, no deadlock:
    #  the waits ended, gpurun_out/standin7_*.log of round 6)
    rccl_standin_ranks(n, "--random", str(seed))


@pytest.mark.gpu
def test_gpu_rccl_rung_bicgstab_and_gmres():
    rccl_standin_ranks(3, "--random", "25", "--asym", "1")
    rccl_standin_ranks(3, "--random", "26", "--gmres", "15")
    rccl_standin_ranks(2, "--shape", "10,10,10", "--procs", "1,1,2", "--renumber", "1")


@pytest.mark.gpu
def test_bench_started_plainly_spawns_its_ranks_and_times_the_rccl_rung():
    """`python bench.py --gpus 2` (no launcher): the parent starts torch.distributed.run as a child before touching the GPU
    and passes rank 0's JSON line through; with the peer mesh switched off the ladder stops at RCCL (the stand-in), whose
    self-test and cross-rank self-check pass."""
    import json
    if not os.path.exists(STANDIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "librccl_standin.so"])
    env = dict(os.environ, OGL_RCCL_LIBRARY=STANDIN, OGL_BENCH_PEER="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--edge", "48", "--iters", "40", "--cpu-iters", "0", "--no-general-legs"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    t = d["config"]["transport"]
    assert t["kind"] == "rccl" and t["rccl_ranks_seen"] == 2, t
    assert (d["config"]["selfcheck"] or {}).get("ok") is True, d["config"]["selfcheck"]
