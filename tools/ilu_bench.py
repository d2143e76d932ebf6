"""IC / ILU / IRILU against BJ(1) on one GPU: generation time, time per apply, iluLevels, iluLaunchesPerApply,
iterations to 1e-6 and time to solution.  Prints one line per (case, preconditioner) and a JSON list at the end.

    python tools/ilu_bench.py [--sizes 64,128,216] [--voronoi 1000000] [--out profiles/<file>.txt]

Times: HIP events around the generation and around 20 back-to-back applies (property precondTimedApplies);
"gen0" includes the pattern-only structure (first solve on a pattern), "gen" is the values-only regeneration of a later
solve.  "solve" = the Krylov loop of a later solve (t_solve_ms), generation NOT included: time to solution is gen + solve."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogl_amd import capi, synthetic  # noqa: E402

KINDS = [("BJ", capi.PRECOND_BJ, capi.SOLVER_CG), ("IC", capi.PRECOND_IC, capi.SOLVER_CG),
         ("ILU", capi.PRECOND_ILU, capi.SOLVER_CG), ("BJ", capi.PRECOND_BJ, capi.SOLVER_BICGSTAB),
         ("IRILU", capi.PRECOND_IRILU, capi.SOLVER_BICGSTAB)]
SOLVER_NAME = {capi.SOLVER_CG: "GKOCG", capi.SOLVER_BICGSTAB: "GKOBiCGStab"}


def run(name, case, lines, rows):
    b = synthetic.apply_case(case, np.ones(case.n_cells))
    for kname, pc, sk in KINDS:
        reg = capi.Registry()
        cfg = capi.default_config(solver=sk, preconditioner=pc, tolerance=1e-6, rel_tol=0.0, max_iter=5000)
        s = reg.solver("f", cfg)
        s.set_property("precondTimedApplies", 20.0)
        s.set_matrix(case)
        s.solve(b, np.zeros_like(b))
        gen0 = s.get_property("precondGenerateMs")
        t0 = time.perf_counter()
        _, perf = s.solve(b, np.zeros_like(b))
        wall = (time.perf_counter() - t0) * 1e3
        get = lambda k: s.get_property(k) if pc >= capi.PRECOND_IC else None  # noqa: E731
        row = dict(case=name, rows=case.n_cells, solver=SOLVER_NAME[sk], precond=kname, gen0_ms=gen0,
                   gen_ms=s.get_property("precondGenerateMs"), apply_ms=s.get_property("precondApplyMs"),
                   levels=get("iluLevels"), launches_per_apply=get("iluLaunchesPerApply"),
                   iterations=perf.n_iterations, solve_ms=perf.t_solve_ms, solve_wall_ms=wall,
                   final_residual=perf.final_residual)
        reg.close()
        rows.append(row)
        line = (f"{name:>12} {SOLVER_NAME[sk]:>11} {kname:>5}  gen0 {gen0:9.2f} ms  gen {row['gen_ms']:9.2f} ms  "
                f"apply {row['apply_ms']:8.3f} ms  levels {row['levels'] or '-':>5}  launches {row['launches_per_apply'] or '-':>5}  "
                f"iters {perf.n_iterations:5d}  solve {perf.t_solve_ms:9.1f} ms")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,216")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, rows = [], []
    for n in [int(v) for v in a.sizes.split(",") if v]:
        run(f"{n}^3", synthetic.poisson_case(n), lines, rows)
    if a.voronoi > 0:
        run(f"voronoi{a.voronoi // 1000}k", synthetic.voronoi_case(a.voronoi), lines, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/ilu_bench.py: IC / ILU / IRILU against BJ(1), tolerance 1e-6 (absolute, rel_tol 0)\n")
            f.write("\n".join(lines) + "\n\n" + json.dumps(rows, indent=1) + "\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
