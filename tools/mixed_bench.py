"""Mixed precision (property mixedPrecision) against the double path under GKOCG + BJ(1) on one GPU: both modes in
alternation on the same box and the same solver handle, after a warm-up solve of each; every solve starts from x = 0
(updateInitGuess 1).

    python tools/mixed_bench.py [--sizes 100,216] [--voronoi 1000000] [--rounds 5] [--out profiles/<file>.txt]

Per case and criterion (relTol 0.01 | the default 1e-6 / 1e-6 | tolerance 1e-10): solve time (t_solve_ms: the loop,
device events and a synchronise at its end; best and median of the rounds), turns and outer steps, microseconds per
turn, and the time of the stand-alone in-loop SpMV of each mode (HIP events around back-to-back launches) with its share
of 8 TB/s on the bytes its model moves: half storage 8 nd + 1 + 16 bytes per row in double and 4 nd + 1 + 8 in single
precision (49 N and 25 N at nd = 4); the CSR arrays 12 nnz + 4 N + 16 N in double and 8 nnz + 4 N + 8 N in single."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogl_amd import capi, synthetic  # noqa: E402

PEAK = 8.0e12  # bytes per second (MI355X HBM3E)
CRITERIA = [("relTol 0.01", dict(tolerance=1e-6, rel_tol=0.01)), ("default 1e-6/1e-6", dict(tolerance=1e-6, rel_tol=1e-6)),
            ("tolerance 1e-10", dict(tolerance=1e-10, rel_tol=0.0))]


def spmv_rows(s, case):
    """The stand-alone SpMV of both modes on this handle: microseconds, modelled bytes, share of peak."""
    n, nnz = case.n_cells, s.dims().local_nnz
    us64 = 1e3 * s.time_spmv(50)
    s.set_property("mixedTimedSpmvs", 50.0)
    s.spmv_f32(np.ones(n, np.float32))
    s.set_property("mixedTimedSpmvs", 0.0)
    us32 = s.get_property("mixedSpmvUs")
    half = s.get_property("mixedInnerLayout") == 2.0
    if half:
        nd = s.get_property("spmvSymPlanes")
        b64, b32, where = (8 * nd + 1 + 16) * n, (4 * nd + 1 + 8) * n, "half storage nd %d" % nd
    else:
        b64, b32, where = 12.0 * nnz + 20.0 * n, 8.0 * nnz + 12.0 * n, "CSR copy"
    double_layout = s.get_property("spmvLayout")
    return dict(inner_layout=where, double_layout=double_layout, spmv64_us=us64, spmv32_us=us32, bytes64=b64, bytes32=b32,
                share64=b64 / (us64 * 1e-6) / PEAK, share32=b32 / (us32 * 1e-6) / PEAK)


def run(name, case, b, rounds, lines, rows):
    reg = capi.Registry()
    for cname, crit in CRITERIA:
        s = reg.solver("p_" + cname.split()[0], capi.default_config(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ,
                                                                  max_block_size=1, max_iter=20000, update_init_guess=1, **crit))
        s.set_matrix(case)
        legs = {0: [], 1: []}
        for rnd in range(rounds + 1):  # round 0 warms both modes up
            for mode in (0, 1):
                s.set_property("mixedPrecision", float(mode))
                x, perf = s.solve(b, np.zeros_like(b))
                if rnd:
                    legs[mode].append(dict(ms=perf.t_solve_ms, turns=perf.n_iterations - 1, res=perf.final_residual,
                                           outer=s.get_property("mixedOuterSteps") if mode else 0,
                                           reason=s.get_property("mixedStopReason") if mode else 0))
        row = dict(case=name, rows=case.n_cells, criterion=cname)
        for mode, tag in ((0, "double"), (1, "mixed")):
            ms = [leg["ms"] for leg in legs[mode]]
            last = legs[mode][-1]
            row[tag] = dict(best_ms=min(ms), median_ms=statistics.median(ms), all_ms=ms, turns=last["turns"],
                            outer=last["outer"], reason=last["reason"], final_residual=last["res"],
                            us_per_turn=1e3 * min(ms) / max(1, last["turns"]))
        row["speedup_best"] = row["double"]["best_ms"] / row["mixed"]["best_ms"]
        if cname == CRITERIA[-1][0]:
            row["spmv"] = spmv_rows(s, case)
        rows.append(row)
        d, m = row["double"], row["mixed"]
        line = (f"{name:>8} {cname:<18} double {d['best_ms']:9.3f} ms (median {d['median_ms']:9.3f}) {d['turns']:5d} turns "
                f"{d['us_per_turn']:7.2f} us/turn | mixed {m['best_ms']:9.3f} ms (median {m['median_ms']:9.3f}) {m['turns']:5d} turns "
                f"{int(m['outer'])} outer, reason {int(m['reason'])} {m['us_per_turn']:7.2f} us/turn | x{row['speedup_best']:.3f}"
                f" | residual {d['final_residual']:.3e} / {m['final_residual']:.3e}")
        if "spmv" in row:
            v = row["spmv"]
            line += (f"\n{name:>8} SpMV ({v['inner_layout']}; double on spmvLayout {v['double_layout']:.0f}): double "
                     f"{v['spmv64_us']:.2f} us = {v['share64']:.3f} of 8 TB/s on {v['bytes64']:.3e} B | single "
                     f"{v['spmv32_us']:.2f} us = {v['share32']:.3f} of 8 TB/s on {v['bytes32']:.3e} B")
        print(line, flush=True)
        lines.append(line)
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,216")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, rows = [], []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        case = synthetic.poisson_case(n)
        run(f"{n}^3", case, synthetic.rhs_for_x_star(case)[0], a.rounds, lines, rows)
    if a.voronoi > 0:
        case = synthetic.voronoi_case(a.voronoi)
        run(f"vor{a.voronoi // 1000}k", case, synthetic.apply_case(case, np.ones(case.n_cells)), a.rounds, lines, rows)
    text = "\n".join(lines) + "\n" + json.dumps(rows) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
