"""The initial guess from the last solutions (keyword guessProjection K) in a time-step loop under
GKOCG + BJ(1) on one GPU, to tolerance 1e-6 (relTol 0 unless --rel-tol): K = 0, 2, 4 and 8, one solver handle each in one
registry, taking every step in alternation on the same box; every handle starts a step from its own last solution, as
OpenFOAM passes it.  The K = 0 leg of the same run is the yardstick.

    python tools/guess_projection_bench.py [--sizes 216,100] [--voronoi 1000000] [--steps 12] [--drift 0.02] [--dt 0.05]
                                           [--legs 0,2,4,8] [--seed 7] [--out profiles/<file>.txt]
                                           [--rel-tol 0.05] [--credit 0|1|both] [--products separate|onePass|alternate]
                                           [--adapt-min-iter 0|1] [--modes 4]

--credit: the keyword guessProjectionCredit on the legs with K > 0 (both: every such K as two legs, as built and credited).
--products: the keyword guessProjectionProducts; alternate: onePass on the odd steps and separate on the even ones of every
leg (the bits are the same, so the loop is the same loop), the products' time of both kinds reported per leg.
--modes N > 4: x*(t) = sum_i sin(w_i t dt + phase_i) u_i over N fixed modes with seeded w_i in (1, 4) -- a field that does
not move inside the span of its last few steps.

The generator (seeded): the mesh's face coefficients move smoothly with the step, upper_f(t) = upper_f (1 + drift sin(0.4 t
+ phase_f)), the diagonal keeps every row's excess over its off-diagonal sum; the right-hand side is A(t) x*(t) for
x*(t) = u0 + (t dt) u1 + (t dt)^2 u2 + sin(3 t dt) u3 with four fixed smooth modes.
Per step and leg: iterations, the wall time of the resident solve (pre-step, solve, post-step; vectors already on the
device), the solve's own time, and the pre-step's time split into products, Gram pass, sums with the small solve, and
update (HIP events, property guessProjectionTimed).  Per leg: the sums over the steps from the third on, and the verdict
against K = 0 -- AHEAD | LOSS only where the leg is on that side in every such step."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ogl_amd import capi, synthetic  # noqa: E402


class Loop:
    """The systems of a time-step loop on one mesh (symmetric, no interfaces)."""

    def __init__(self, case, drift, dt, seed, modes=4):
        assert case.lower is None and not case.interfaces
        self.case, self.drift, self.dt = case, drift, dt
        rng = np.random.default_rng(seed)
        n, lo, up = case.n_cells, case.lower_addr, case.upper_addr
        self.phase = rng.uniform(0.0, 2.0 * np.pi, lo.size)
        self.excess = case.diag - np.bincount(lo, np.abs(case.upper), n) - np.bincount(up, np.abs(case.upper), n)
        g = np.arange(n, dtype=np.float64) / n
        self.modes = [np.sin(2.0 * np.pi * (i + 1) * g) * (1.0 + i * g) + 0.01 * rng.standard_normal(n) for i in range(4)]
        for i in range(4, modes):
            self.modes.append(np.sin(2.0 * np.pi * (i + 1) * g + i) * (1.0 + 0.1 * i * g))
        self.omega, self.shift = rng.uniform(1.0, 4.0, modes), rng.uniform(0.0, 2.0 * np.pi, modes)

    def system(self, t):
        c, n = self.case, self.case.n_cells
        upper = c.upper * (1.0 + self.drift * np.sin(0.4 * t + self.phase))
        diag = self.excess + np.bincount(c.lower_addr, np.abs(upper), n) + np.bincount(c.upper_addr, np.abs(upper), n)
        case = synthetic.LduCase(n, c.lower_addr, c.upper_addr, diag, upper, None)
        s, U = t * self.dt, self.modes
        if len(U) == 4:
            x = U[0] + s * U[1] + s * s * U[2] + np.sin(3.0 * s) * U[3]
        else:
            x = sum(np.sin(w * s + ph) * u for w, ph, u in zip(self.omega, self.shift, U))
        b = diag * x + np.bincount(c.lower_addr, upper * x[c.upper_addr], n) + np.bincount(c.upper_addr, upper * x[c.lower_addr], n)
        return capi.LduArrays(case), b


def run(name, case, a, lines):
    """A leg is (K, credit); the first one is the yardstick."""
    legs = []
    for K in (int(k) for k in a.legs.split(",")):
        for credit in ((0, 1) if a.credit == "both" and K else (int(a.credit == "1") if K else 0,)):
            legs.append((K, credit))
    tag = {leg: f"K {leg[0]}" + (" credited" if leg[1] else "") for leg in legs}
    loop = Loop(case, a.drift, a.dt, a.seed, a.modes)
    reg = capi.Registry()
    cfg = capi.default_config(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ, max_block_size=1, tolerance=1e-6,
                              rel_tol=a.rel_tol, max_iter=5000, update_init_guess=1, adapt_min_iter=a.adapt_min_iter)
    handles = {leg: reg.solver(f"p{leg[0]}c{leg[1]}", cfg) for leg in legs}
    xs = {leg: np.zeros(case.n_cells) for leg in legs}
    rows = {leg: [] for leg in legs}
    for t in range(a.steps):
        arrays, b = loop.system(t)
        products = a.products if a.products != "alternate" else ("onePass" if t % 2 else "separate")
        for leg in legs:
            K, credit = leg
            s = handles[leg].set_matrix(arrays)
            s.set_guess_projection(K).set_guess_projection_credit(credit).set_guess_projection_products(products)
            s.set_property("guessProjectionTimed", 1.0)
            s.upload_rhs(b)
            s.upload_solution(xs[leg])
            t0 = time.perf_counter()
            perf = s.apply_resident()
            wall = (time.perf_counter() - t0) * 1e3
            xs[leg] = s.download_solution()
            offered = int(s.get_property("guessProjectionOffered")) if K else 0
            split = [s.get_property(f"guessProjection{p}Ms") if offered else 0.0 for p in ("Products", "Gram", "Solve", "Update")]
            one_pass = int(s.get_property("guessProjectionOnePassInUse")) if offered else 0
            row = dict(its=perf.n_iterations, wall=wall, solve=perf.t_solve_ms, split=split, offered=offered, one_pass=one_pass,
                       kept=int(s.get_property("guessProjectionKept")) if K else 0, res=perf.final_residual,
                       init=perf.initial_residual)
            if credit and offered and s.get_property("guessProjectionCreditInUse"):  # the contract, on whatever turn shape ran
                assert perf.initial_residual == s.get_property("guessProjectionNormBefore") / perf.norm_factor
            rows[leg].append(row)
            line = (f"{name:>10} step {t:2d} {tag[leg]}: {row['its']:5d} iterations, resident solve {wall:9.3f} ms (solve itself "
                    f"{row['solve']:9.3f}), offered {offered} kept {row['kept']}, pre-step {sum(split):7.3f} ms = products "
                    f"{split[0]:.3f} ({'one pass' if one_pass else 'separate'}) + Gram {split[1]:.3f} + sums and small solve "
                    f"{split[2]:.3f} + update {split[3]:.3f}; residual {row['init']:.2e} -> {row['res']:.2e}")
            print(line, flush=True)
            lines.append(line)
    base = rows[legs[0]]
    for leg in legs:
        r = rows[leg][2:]
        its, wall = sum(v["its"] for v in r), sum(v["wall"] for v in r)
        line = f"{name:>10} {tag[leg]}, steps 2 .. {a.steps - 1}: {its} iterations, {wall:.2f} ms of resident solves"
        if leg != legs[0]:
            b_its, b_wall = sum(v["its"] for v in base[2:]), sum(v["wall"] for v in base[2:])
            ahead = all(v["wall"] < w["wall"] for v, w in zip(r, base[2:]))
            behind = all(v["wall"] > w["wall"] for v, w in zip(r, base[2:]))
            line += (f" -- against {tag[legs[0]]}: iterations x{its / b_its:.3f}, time x{wall / b_wall:.3f}, "
                     f"{'AHEAD' if ahead else 'LOSS' if behind else 'mixed'} (ahead in "
                     f"{sum(v['wall'] < w['wall'] for v, w in zip(r, base[2:]))} of {len(r)} steps)")
            # the products of the pre-step at a full ring (k = K), by kind
            full = [v for v in r if v["offered"] == leg[0]]
            for kind, flag in (("separate", 0), ("one pass", 1)):
                ms = [v["split"][0] for v in full if v["one_pass"] == flag]
                if ms:
                    line += f"; products {kind} at k = {leg[0]}: median {np.median(ms):.3f} ms over {len(ms)} steps"
        print(line, flush=True)
        lines.append(line)
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="216,100")
    ap.add_argument("--voronoi", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--drift", type=float, default=0.02)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--legs", default="0,2,4,8")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rel-tol", type=float, default=0.0)
    ap.add_argument("--credit", choices=("0", "1", "both"), default="0")
    ap.add_argument("--products", choices=("separate", "onePass", "alternate"), default="separate")
    ap.add_argument("--adapt-min-iter", type=int, choices=(0, 1), default=1)
    ap.add_argument("--modes", type=int, default=4)
    a = ap.parse_args()
    lines = [f"# relTol {a.rel_tol}, credit {a.credit}, products {a.products}, adaptMinIter {a.adapt_min_iter}, "
             f"{a.modes} modes, {a.steps} steps, legs {a.legs}"]
    for n in [int(v) for v in a.sizes.split(",") if v]:
        run(f"{n}^3", synthetic.poisson_case(n), a, lines)
    if a.voronoi > 0:
        run(f"voronoi{a.voronoi // 1000}k", synthetic.voronoi_case(a.voronoi), a, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
