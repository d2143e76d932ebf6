#!/usr/bin/env python3
"""A/B of two builds of libogl_amd.so on one box: runs bench.py alternately with the in-tree library
and with another one (e.g. tools/bin/libogl_amd_<commit>.so built from an earlier commit) and prints
the in-loop SpMV time and the turn rate of every run.  Development tool.

  python tools/ab_bench.py tools/bin/libogl_amd_2c97ef6.so [rounds] [bench.py flags ...]

OGL_AB_IN_TREE_PROP="KEY=v1,v2,..." runs the in-tree library once per value in every round, with --prop KEY=v (the other
library never sees the property: it may not know it).

Every run is a child process with a time limit of its own (OGL_AB_TIMEOUT_S, 300 s by default).  The first run that
fails -- a non-zero exit, a time-out, no result line -- ends the whole A/B with exit status 1: nothing more is started on
a device that a run may have left in a bad state.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
other = os.path.abspath(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
flags = sys.argv[3:]
limit = float(os.environ.get("OGL_AB_TIMEOUT_S", "300"))
runner = ("import sys, runpy; sys.path.insert(0, %r); from ogl_amd import capi; capi.LIB_PATH = sys.argv[1]; "
          "sys.argv = ['bench.py'] + sys.argv[2:]; runpy.run_path(%r, run_name='__main__')"
          % (ROOT, os.path.join(ROOT, "bench.py")))
in_tree = os.path.join(ROOT, "ogl_amd", "lib", "libogl_amd.so")
libs = [("in-tree", in_tree, [])]
if os.environ.get("OGL_AB_IN_TREE_PROP"):
    key, values = os.environ["OGL_AB_IN_TREE_PROP"].split("=")
    libs = [("in-tree %s=%s" % (key, v), in_tree, ["--prop", "%s=%s" % (key, v)]) for v in values.split(",")]
libs.append((os.path.basename(other), other, []))
for r in range(rounds):
    for name, lib, extra in libs:
        cmd = [sys.executable, "-c", runner, lib, "--steps", "3", "--warmup", "1", "--cpu-iters", "0", "--no-general-legs", *flags,
               *extra]
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("round %d %-28s TIMED OUT after %g s: stopping" % (r, name, limit), flush=True)
            sys.exit(1)
        if p.returncode != 0:
            print("round %d %-28s FAILED with exit status %d: stopping\n%s" % (r, name, p.returncode, p.stderr[-800:]), flush=True)
            sys.exit(1)
        try:
            d = json.loads(p.stdout.strip().splitlines()[-1])
            ms = d["roofline"]["avg_kernel_ms"]  # None where no turn is event-timed (--no-profile)
            print("round %d %-28s %8.1f it/s  spmv %s us  layout %s" % (
                r, name, d["value"], "%6.1f" % (1e3 * ms) if ms is not None else "   n/a", d["roofline"]["layout"]), flush=True)
        except Exception as e:
            print("round %d %-28s NO RESULT LINE (%s): stopping\n%s" % (r, name, e, p.stderr[-800:]), flush=True)
            sys.exit(1)
