"""Preconditioner Chebyshev against BJ(1) on one GPU: time per apply and per step beside the in-loop
product's time of the same run, iterations to 1e-6 and time per solve.  Prints one line per (case, leg) and a JSON list at
the end.

    python tools/chebyshev_bench.py [--sizes 100,216] [--voronoi 1000000] [--degrees 1,2,3,4] [--gmres-sizes 216]
                                    [--rounds 5] [--out profiles/<file>.txt]

Legs per case: GKOCG with BJ(1) and with Chebyshev of every degree, fused and unfused (property chebyshevFused; on a layout
other than the whole-matrix half storage both run unfused and only one is kept); for the sizes of --gmres-sizes also
GKOGMRES(30) with orthoMethod cgs under BJ(1) and under Chebyshev of degree 4.

Protocol: every leg keeps its own registry and solver; after two warm-up solves each (the second also times 20 back-to-back
applies with HIP events, property precondTimedApplies, and the in-loop product, ogl_solver_time_spmv), `rounds` rounds run
the legs one after the other, so that every leg's solves are spread over the whole run; a leg's figure is the median of its
rounds' Krylov-loop times (t_solve_ms: generation not included; gen_ms beside it), min and max are kept."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogl_amd import capi, synthetic  # noqa: E402


class Leg:
    def __init__(self, case, b, solver, name, degree=0, fused=1):
        self.name, self.degree, self.b = name, degree, b
        kw = dict(krylov_dim=30) if solver == capi.SOLVER_GMRES else {}
        cfg = capi.default_config(solver=solver, preconditioner=capi.PRECOND_CHEBYSHEV if degree else capi.PRECOND_BJ,
                                  tolerance=1e-6, rel_tol=0.0, max_iter=5000, **kw)
        self.reg = capi.Registry()
        self.s = self.reg.solver("f", cfg)
        if solver == capi.SOLVER_GMRES:
            self.s.set_ortho_method("cgs")
        if degree:
            self.s.set_chebyshev(degree=degree)
            self.s.set_property("chebyshevFused", float(fused))
        self.s.set_property("precondTimedApplies", 20.0)
        self.s.set_matrix(case)
        self.s.solve(b, np.zeros_like(b))  # (the first solve allocates the vectors the timed applies run on)
        _, perf = self.s.solve(b, np.zeros_like(b))
        self.row = dict(leg=name, degree=degree, iterations=perf.n_iterations, final_residual=perf.final_residual,
                        apply_us=1e3 * self.s.get_property("precondApplyMs") if degree else None,
                        gen_ms=self.s.get_property("precondGenerateMs"), spmv_us=1e3 * self.s.time_spmv(20),
                        fused_in_use=self.s.get_property("chebyshevFusedInUse") if degree else None,
                        launches_per_apply=self.s.get_property("chebyshevLaunchesPerApply") if degree else None,
                        lambda_max=self.s.get_property("chebyshevLambdaMaxInUse") if degree else None,
                        layout=self.s.get_property("spmvLayout"), half=self.s.get_property("symmetricHalf"))
        self.s.set_property("precondTimedApplies", 0.0)
        self.times = []

    def round(self):
        _, perf = self.s.solve(self.b, np.zeros_like(self.b))
        self.row["iterations"] = perf.n_iterations  # (with adaptMinIter the first check falls where the last solve's count puts it)
        self.times.append(perf.t_solve_ms)

    def finish(self):
        self.reg.close()
        t = self.times
        self.row.update(solve_ms=statistics.median(t), solve_ms_min=min(t), solve_ms_max=max(t), rounds=len(t))
        if self.degree:
            self.row["step_us"] = self.row["apply_us"] / self.degree  # (the first launch's share included)
            self.row["step_over_spmv"] = self.row["step_us"] / self.row["spmv_us"]
        return self.row


def run(name, case, lines, rows, a, gmres):
    b = synthetic.apply_case(case, np.ones(case.n_cells))
    legs = [Leg(case, b, capi.SOLVER_CG, "GKOCG BJ(1)")]
    for d in [int(v) for v in a.degrees.split(",")]:
        fused = Leg(case, b, capi.SOLVER_CG, f"GKOCG Cheb({d}) fused", d, 1)
        legs.append(fused)
        if fused.row["fused_in_use"] == 1.0:
            legs.append(Leg(case, b, capi.SOLVER_CG, f"GKOCG Cheb({d}) unfused", d, 0))
        else:
            fused.name = fused.row["leg"] = f"GKOCG Cheb({d}) unfused"
    if gmres:
        legs.append(Leg(case, b, capi.SOLVER_GMRES, "GKOGMRES(30) cgs BJ(1)"))
        legs.append(Leg(case, b, capi.SOLVER_GMRES, "GKOGMRES(30) cgs Cheb(4)", 4, 1))
    for _ in range(a.rounds):
        for leg in legs:
            leg.round()
    for leg in legs:
        r = leg.finish()
        r.update(case=name, rows=case.n_cells)
        rows.append(r)
        apply = f"apply {r['apply_us']:8.1f} us  step {r['step_us']:7.1f} us = {r['step_over_spmv']:.2f} x" if r["degree"] else " " * 50
        line = (f"{name:>12} {r['leg']:>26}  spmv {r['spmv_us']:7.1f} us  {apply}  gen {r['gen_ms']:7.3f} ms  "
                f"iters {r['iterations']:5d}  solve {r['solve_ms']:9.2f} ms [{r['solve_ms_min']:.2f} .. {r['solve_ms_max']:.2f}]")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,216")
    ap.add_argument("--gmres-sizes", default="216")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--degrees", default="1,2,3,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, rows = [], []
    gmres_sizes = [int(v) for v in a.gmres_sizes.split(",") if v]
    for n in [int(v) for v in a.sizes.split(",") if v]:
        run(f"{n}^3", synthetic.poisson_case(n), lines, rows, a, n in gmres_sizes)
    if a.voronoi > 0:
        run(f"voronoi{a.voronoi // 1000}k", synthetic.voronoi_case(a.voronoi), lines, rows, a, False)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/chebyshev_bench.py: Chebyshev against BJ(1), tolerance 1e-6 (absolute, rel_tol 0); solve = median of "
                    f"{a.rounds} alternating rounds [min .. max]\n")
            f.write("\n".join(lines) + "\n\n" + json.dumps(rows, indent=1) + "\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
