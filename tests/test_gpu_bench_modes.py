"""bench.py's two kinds of run on a small box: a plain run does set-up, warm-up, the timed steps and the result line and
nothing else; --full adds the figures besides the headline (here the general legs, the PCIe-inclusive call and the
momentum components; the CPU baselines and the live PMC passes are switched off to keep the test short)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(*flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--edge", "32", "--iters", "20", *flags], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_gpu_bench_plain_run_is_the_headline_only_and_full_adds_the_rest():
    plain = bench()
    assert plain["metric"] == "cg_iters_per_sec" and plain["unit"] == "iter/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f64" and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["roofline"]["avg_kernel_ms"] > 0 and plain["roofline"]["traffic_measured_in_this_run"] is False
    assert plain["roofline_general"] is None and "cpu_baseline" not in plain
    assert "solve_incl_pcie_s" not in plain["boundary"] and plain["boundary"]["momentum_components"] is None

    full = bench("--full", "--cpu-iters", "0", "--live-pmc", "off")
    assert full["value"] > 0 and full["roofline"]["avg_kernel_ms"] > 0
    assert [g["leg"] for g in full["roofline_general"]] == ["full_storage", "no_compress", "shuffle65536"]
    assert full["boundary"]["solve_incl_pcie_s"] > 0 and full["boundary"]["iters_per_sec_incl_pcie"] > 0
    assert full["boundary"]["momentum_components"] is not None

    # --no-profile: the separate SpMV loop is a figure of its own, --full only
    np_plain = bench("--no-profile")
    assert np_plain["value"] > 0 and np_plain["roofline"]["avg_kernel_ms"] is None
    assert np_plain["roofline"]["achieved"] is None and np_plain["roofline"]["frac"] is None
    np_full = bench("--no-profile", "--full", "--cpu-iters", "0")
    assert np_full["roofline"]["avg_kernel_ms"] > 0 and np_full["roofline"]["frac"] > 0
