"""IC / ILU / IRILU against BJ(1) on one GPU: generation time, time per apply, iluLevels, iluLaunchesPerApply,
iterations to 1e-6 and time to solution.  Prints one line per (case, preconditioner) and a JSON list at the end.

    python tools/ilu_bench.py [--sizes 64,128,216] [--voronoi 1000000] [--out profiles/<file>.txt]
                              [--triangular-solves exact,isai] [--factor-sweeps 0,3] [--sparsity-power 1,2]

The three leg options (keywords triangularSolves, factorSweeps, sparsityPower of IC / ILU) multiply
the IC and ILU rows: every combination runs in the same process as the BJ(1) and the exact rows it is judged against
(sparsityPower only matters under isai).  Their defaults -- exact, 0, 1 -- are the parent's rows alone.

Times: HIP events around the generation and around 20 back-to-back applies (property precondTimedApplies);
"gen0" includes the pattern-only structure (first solve on a pattern), "gen" is the generation of the second solve --
without `caching` it goes into the field's own object, so it builds the pattern-only structure once more; only a third
solve would be values-only.  "solve" = the Krylov loop of a later solve (t_solve_ms), generation NOT included: time to solution is gen + solve."""
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


def legs_of(pc, a):
    """(triangularSolves, factorSweeps, sparsityPower) legs of a kind: IC and ILU take all of them, IRILU the sweeps."""
    if pc not in (capi.PRECOND_IC, capi.PRECOND_ILU, capi.PRECOND_IRILU):
        return [("exact", 0, 1)]
    out = []
    for tri in a.triangular_solves.split(","):
        if tri == "isai" and pc == capi.PRECOND_IRILU:
            continue
        for sweeps in [int(v) for v in a.factor_sweeps.split(",")]:
            for power in [int(v) for v in a.sparsity_power.split(",")] if tri == "isai" else [1]:
                out.append((tri, sweeps, power))
    return out


def run(name, case, lines, rows, a):
    b = synthetic.apply_case(case, np.ones(case.n_cells))
    for kname, pc, sk, tri, sweeps, power in [k + leg for k in KINDS for leg in legs_of(k[1], a)]:
        reg = capi.Registry()
        cfg = capi.default_config(solver=sk, preconditioner=pc, tolerance=1e-6, rel_tol=0.0, max_iter=5000,
                                  sparsity_power=power)
        s = reg.solver("f", cfg)
        s.set_property("precondTimedApplies", 20.0)
        s.set_triangular_solves(tri).set_factor_sweeps(sweeps)
        if (tri, sweeps) != ("exact", 0):
            kname = f"{kname}/{tri}" + (f",p{power}" if tri == "isai" else "") + (f",s{sweeps}" if sweeps else "")
        s.set_matrix(case)
        try:
            s.solve(b, np.zeros_like(b))
            gen0 = s.get_property("precondGenerateMs")
            t0 = time.perf_counter()
            _, perf = s.solve(b, np.zeros_like(b))
            wall = (time.perf_counter() - t0) * 1e3
        except capi.OglError as e:  # (a row of W wider than the kernel takes: the leg is recorded as refused)
            reg.close()
            line = f"{name:>12} {SOLVER_NAME[sk]:>11} {kname:>14}  refused: {e}"
            print(line, flush=True)
            lines.append(line)
            rows.append(dict(case=name, rows=case.n_cells, solver=SOLVER_NAME[sk], precond=kname, refused=str(e)))
            continue
        get = lambda k: s.get_property(k) if pc >= capi.PRECOND_IC else None  # noqa: E731
        row = dict(case=name, rows=case.n_cells, solver=SOLVER_NAME[sk], precond=kname, gen0_ms=gen0,
                   gen_ms=s.get_property("precondGenerateMs"), apply_ms=s.get_property("precondApplyMs"),
                   levels=get("iluLevels"), launches_per_apply=get("iluLaunchesPerApply"),
                   triangular_solves=tri, factor_sweeps=sweeps, sparsity_power=power, w_entries=get("triangularWEntries"),
                   iterations=perf.n_iterations, solve_ms=perf.t_solve_ms, solve_wall_ms=wall,
                   final_residual=perf.final_residual)
        reg.close()
        rows.append(row)
        line = (f"{name:>12} {SOLVER_NAME[sk]:>11} {kname:>14}  gen0 {gen0:9.2f} ms  gen {row['gen_ms']:9.2f} ms  "
                f"apply {row['apply_ms']:8.3f} ms  levels {row['levels'] or '-':>5}  launches {row['launches_per_apply'] or '-':>5}  "
                f"iters {perf.n_iterations:5d}  solve {perf.t_solve_ms:9.1f} ms")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,216")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--triangular-solves", default="exact")
    ap.add_argument("--factor-sweeps", default="0")
    ap.add_argument("--sparsity-power", default="1")
    a = ap.parse_args()
    lines, rows = [], []
    for n in [int(v) for v in a.sizes.split(",") if v]:
        run(f"{n}^3", synthetic.poisson_case(n), lines, rows, a)
    if a.voronoi > 0:
        run(f"voronoi{a.voronoi // 1000}k", synthetic.voronoi_case(a.voronoi), lines, rows, a)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/ilu_bench.py: IC / ILU / IRILU against BJ(1), tolerance 1e-6 (absolute, rel_tol 0)\n")
            f.write("\n".join(lines) + "\n\n" + json.dumps(rows, indent=1) + "\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
