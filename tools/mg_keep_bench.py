"""Multigrid's keyword aggregateCaching ("kept aggregates") in a time-step loop on one GPU: the legs
`aggregateCaching 0` (every solve a full generation: the yardstick) and `aggregateCaching N` (one full generation, then
refreshes of the values under its aggregates) in alternation on one handle and one right-hand side, with BJ(1) on the same
box as the line to beat.  A leg is --steps solves of GKOCG at tolerance 1e-6 from x = 0; the coefficients of step t are the
case's with every third row's diagonal scaled by 1 + drift t, and all legs of a round see the same steps, so their
iteration counts compare solve by solve.  Two solves that are not counted go in front of every leg: one with
aggregateCaching 0 (nothing of the leg before is reused), one on step 0's coefficients with the leg's keyword -- the N
leg's full generation.  Every counted step of the N leg is then a refresh under the aggregates of step 0: current at step 0,
t steps old at step t.

    python tools/mg_keep_bench.py [--sizes 100,160,216] [--voronoi 1000000] [--variants hashed:3,pgm:1]
                                  [--precision double,single] [--drift 0.02] [--keep 10] [--steps 6] [--rounds 5]
                                  [--adapt-min-iter 0|1] [--out profiles/<file>.txt]

--adapt-min-iter 1 (the default, as a case runs): a solve iterates at least relaxationFactor (0.6) times as often as the one
before it on the same handle and checks the residual at the adaptive frequency, so on coefficients that get easier the
iteration counts of all legs follow that floor.  0 switches both off (a check per iteration): the counts are then what the
preconditioner needs, which is how the iterations that stale aggregates cost are read.

Per leg: precondGenerateMs (HIP events around the generation) of the full generations and of the refreshes, and per step
(the median of the rounds) iterations, loop (t_solve_ms) and solve (generation + loop); per round the sum of the steps' solve
times; mgKeptBytes.  hashed/3 also runs with one sweep and correctionScale 1.5, and the first variant once more with the maps
loaded past the caches (property mgKeepStream 1).  A gain is claimed only where the new leg is ahead of the yardstick in
every round and by more than twice the spread of the yardstick's rounds: the N leg against the 0 leg on a
round's sum, and step by step the N leg against BJ(1)."""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogl_amd import capi, synthetic  # noqa: E402


def step_case(case, drift, t):
    c = copy.copy(case)
    c.diag = case.diag.copy()
    c.diag[::3] *= 1.0 + drift * t
    return c


def leg(s, cases, b, keep, stream):
    """One leg on the handle: per step (generation ms, refreshed?, iterations, loop ms)."""
    s.set_property("mgKeepStream", 1.0 if stream else 0.0)
    for k in (0, keep):  # (not counted)
        s.set_multigrid(aggregateCaching=k)
        s.set_matrix(cases[0])
        s.solve(b, np.zeros_like(b))
    out = []
    for c in cases:
        s.set_matrix(c)
        _, perf = s.solve(b, np.zeros_like(b))
        out.append((s.get_property("precondGenerateMs"), s.get_property("mgAggregatesReused") == 1.0, perf.n_iterations,
                    perf.t_solve_ms))
    return out


def ahead(new, base):
    """new and base: one time per round.  The rule of DESIGN section 7e."""
    return all(n < o for n, o in zip(new, base)) and min(base) - max(new) > 2.0 * (max(base) - min(base))


def summary(rounds):
    """rounds: per round the steps of a leg."""
    med = statistics.median
    full = [x[0] for r in rounds for x in r if not x[1]]
    fresh = [x[0] for r in rounds for x in r if x[1]]
    steps = range(len(rounds[0]))
    return dict(gen_full_ms=med(full) if full else None, gen_refresh_ms=med(fresh) if fresh else None,
                gen_refresh_min_ms=min(fresh) if fresh else None, refreshes=len(fresh), full_generations=len(full),
                iterations=[int(med(r[t][2] for r in rounds)) for t in steps],
                loop_ms=[med(r[t][3] for r in rounds) for t in steps],
                solve_ms=[med(r[t][0] + r[t][3] for r in rounds) for t in steps],
                solve_rounds_ms=[[r[t][0] + r[t][3] for r in rounds] for t in steps],
                round_ms=[sum(x[0] + x[3] for x in r) for r in rounds])


def fmt(v):
    return "[" + " ".join(f"{x:.2f}" for x in v) + "]"


def run(name, case, variants, a, emit):
    b = synthetic.apply_case(case, np.ones(case.n_cells))
    reg = capi.Registry()
    steps = [step_case(case, a.drift, t) for t in range(a.steps)]
    cfg = dict(solver=capi.SOLVER_CG, tolerance=1e-6, rel_tol=0.0, max_iter=5000, renumber=capi.RENUMBER_OFF,
               adapt_min_iter=a.adapt_min_iter)
    bj = reg.solver("bj", capi.default_config(preconditioner=capi.PRECOND_BJ, **cfg))
    bj.set_property("precondTimedApplies", 1.0)
    bj_rounds = []

    def bj_round():
        r = []
        for c in steps:
            bj.set_matrix(c)
            _, perf = bj.solve(b, np.zeros_like(b))
            r.append((bj.get_property("precondGenerateMs"), False, perf.n_iterations, perf.t_solve_ms))
        return r

    bj_round()
    for k, v in enumerate(variants):
        s = reg.solver(f"mg{k}", capi.default_config(preconditioner=capi.PRECOND_MULTIGRID, caching=0, **cfg))
        s.set_multigrid(aggregation=v[0], aggregatePasses=v[1], cyclePrecision=v[2], smootherSweeps=v[3], correctionScale=v[4])
        s.set_property("precondTimedApplies", 1.0)  # (times the generation; one apply more per solve, outside t_solve_ms)
        legs = [("0", 0, False), (str(a.keep), a.keep, False)] + ([(f"{a.keep}s", a.keep, True)] if k == 0 else [])
        got = {w: [] for w, _, _ in legs}
        for rnd in range(a.rounds + 1):  # (round 0: the warm-up of each leg)
            for w, keep, stream in legs:
                r = leg(s, steps, b, keep, stream)
                if rnd > 0:
                    got[w].append(r)
            if rnd > 0:
                bj_rounds.append(bj_round())
        kept_bytes = s.get_property("mgKeptBytes")
        label = f"{v[0]}/{v[1]} {v[2]} sweeps {v[3]} scale {v[4]:g}"
        rows = {w: summary(r) for w, r in got.items()}
        bj_row = summary(bj_rounds[-a.rounds:])
        for w, row in rows.items():
            emit(dict(case=name, rows=case.n_cells, variant=label, leg=w, kept_bytes=kept_bytes, drift=a.drift, **row),
                 f"{name:>9} {label:>36} aggregateCaching {w:>4}  gen full "
                 + (f"{row['gen_full_ms']:8.3f} ms" if row['gen_full_ms'] is not None else "       - ") + "  refresh "
                 + (f"{row['gen_refresh_ms']:7.3f} (min {row['gen_refresh_min_ms']:.3f}) ms" if row['gen_refresh_ms'] is not None
                    else "      -") +
                 f"  iters {row['iterations']}  loop {fmt(row['loop_ms'])}  solve {fmt(row['solve_ms'])} ms  "
                 f"round {fmt(row['round_ms'])} ms  kept {kept_bytes / 2 ** 20:.1f} MiB")
        base, new = rows["0"], rows[str(a.keep)]
        gain = ahead(new["round_ms"], base["round_ms"])
        beats = [t for t in range(a.steps) if ahead(new["solve_rounds_ms"][t], bj_row["solve_rounds_ms"][t])]
        emit(dict(case=name, variant=label, gain_claimed=gain, steps_ahead_of_bj=beats),
             f"{name:>9} {label:>36} a round of {a.steps} steps {statistics.median(base['round_ms']):.2f} -> "
             f"{statistics.median(new['round_ms']):.2f} ms (yardstick spread "
             f"{max(base['round_ms']) - min(base['round_ms']):.2f} ms): gain {'claimed' if gain else 'not claimed'};  "
             f"BJ(1) solve {fmt(bj_row['solve_ms'])} ms, iters {bj_row['iterations']}: aggregateCaching {a.keep} ahead of it at "
             f"steps {beats if beats else 'none'}")
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,160,216")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--variants", default="hashed:3,pgm:1")
    ap.add_argument("--precision", default="double,single")
    ap.add_argument("--drift", type=float, default=0.02)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--adapt-min-iter", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    variants = []
    for g in [g for g in a.variants.split(",") if g]:
        word, _, passes = g.partition(":")
        variants += [(word, int(passes or 1), p, 2, 1.0) for p in a.precision.split(",") if p]
        if word == "hashed" and int(passes or 1) == 3:
            variants.append((word, 3, a.precision.split(",")[-1], 1, 1.5))
    rows = []

    def emit(row, line):
        rows.append(row)
        print(line, flush=True)
        if a.out:  # (line by line: a run that is cut short leaves what it measured)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for n in [int(x) for x in a.sizes.split(",") if x]:
        run(f"{n}^3", synthetic.poisson_case(n), variants, a, emit)
    if a.voronoi > 0:
        run(f"vor{a.voronoi // 1000}k", synthetic.voronoi_case(a.voronoi), variants, a, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
