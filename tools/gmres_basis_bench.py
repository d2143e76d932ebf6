"""The stored precision of GKOGMRES' Krylov basis (property basisPrecision: double | single) under
GKOGMRES(30) + BJ(1) on one GPU: orthoMethod cgs and cgs2, each on a double and on a single basis, the four legs in
alternation on the same box and the same solver handle, after a warm-up solve of each; every solve starts from x = 0
(updateInitGuess 1) and runs to tolerance 1e-6 (relTol 0) or --max-iter, whichever comes first.  The double legs of the
same run are the yardstick.

    python tools/gmres_basis_bench.py [--sizes 100,216] [--asym 126] [--big 368] [--rounds 5] [--max-iter 2000]
                                      [--out profiles/<file>.txt]

Per case and leg: solve time (t_solve_ms; every round, best and median), turns, microseconds per turn, the recorded
residual and the true one (sum |b - A x| / norm factor, formed on the host from the LDU arrays).  Per case and method the
verdict: single is AHEAD only where its solve time is below the double leg's in every round and the gap of the medians is
more than twice the spread (max - min) of the double legs; otherwise level, or a loss by the same rule the other way round.
Per case: the block kernels alone (property orthoTimedLaunches: HIP events around back-to-back launches on the solve's
own buffers) at columns it = 0, 15 and 29 on both bases, with their share of 8 TB/s on the bytes the model moves, k = it
+ 1 basis vectors of e = 8 | 4 bytes per entry: multidot 8 N + e N k, the update 16 N + e N k (with cgs2's second-round
partials, "UpdateDots", the rows of V are held in registers for up to 32 vectors, so the bytes are the same)."""
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
LEGS = [(m, p) for m in ("cgs", "cgs2") for p in ("double", "single")]
KRYLOV_DIM = 30


def true_residual(case, b, x, norm_factor):
    return float(np.sum(np.abs(b - synthetic.apply_case(case, x)))) / norm_factor


def kernel_rows(s, case, b):
    """The block kernels alone on either basis, after a short cgs2 solve that leaves the buffers behind."""
    n = case.n_cells
    out = []
    for basis, e in (("double", 8.0), ("single", 4.0)):
        s.set_ortho_method("cgs2").set_basis_precision(basis)
        s.set_property("orthoTimedLaunches", 20.0)
        s.solve(b, np.zeros_like(b))
        s.set_property("orthoTimedLaunches", 0.0)
        assert s.get_property("basisPrecisionInUse") == capi.BASIS_PRECISION[basis]
        for it in (0, 15, 29):
            k = it + 1
            for key, bytes_moved in (("orthoMultidotUs", 8.0 * n + e * n * k), ("orthoUpdateUs", 16.0 * n + e * n * k),
                                     ("orthoUpdateDotsUs", 16.0 * n + e * n * k)):
                us = s.get_property(f"{key}_{it}")
                out.append(dict(kernel=key[5:-2], basis=basis, it=it, us=us, bytes=bytes_moved,
                                share=bytes_moved / (us * 1e-6) / PEAK))
    return out


def verdict(double_ms, single_ms):
    """AHEAD | LOSS only when every round agrees and the medians are more than twice the double legs' spread apart."""
    spread = max(double_ms) - min(double_ms)
    gap = statistics.median(double_ms) - statistics.median(single_ms)
    if all(s < d for s, d in zip(single_ms, double_ms)) and gap > 2.0 * spread:
        return "AHEAD"
    if all(s > d for s, d in zip(single_ms, double_ms)) and -gap > 2.0 * spread:
        return "LOSS"
    return "level"


def run(name, case, b, rounds, max_iter, lines, rows):
    reg = capi.Registry()
    s = reg.solver("p", capi.default_config(solver=capi.SOLVER_GMRES, preconditioner=capi.PRECOND_BJ, max_block_size=1,
                                            krylov_dim=KRYLOV_DIM, tolerance=1e-6, rel_tol=0.0, max_iter=max_iter,
                                            update_init_guess=1))
    s.set_matrix(case)
    legs = {leg: [] for leg in LEGS}
    x_last = {}
    for rnd in range(rounds + 1):  # round 0 warms every leg up
        for leg in LEGS:
            s.set_ortho_method(leg[0]).set_basis_precision(leg[1])
            x, perf = s.solve(b, np.zeros_like(b))
            assert s.get_property("orthoMethodInUse") == capi.ORTHO_METHOD[leg[0]]
            assert s.get_property("basisPrecisionInUse") == capi.BASIS_PRECISION[leg[1]]
            if rnd:
                legs[leg].append(dict(ms=perf.t_solve_ms, turns=perf.n_iterations - 1, res=perf.final_residual,
                                      norm_factor=perf.norm_factor, basis_bytes=s.get_property("basisBytes")))
                x_last[leg] = x
            print(f"# {name} round {rnd} {leg[0]} {leg[1]}: {perf.t_solve_ms:.3f} ms, {perf.n_iterations - 1} turns", flush=True)
    row = dict(case=name, rows=case.n_cells, krylov_dim=KRYLOV_DIM, max_iter=max_iter)
    for leg in LEGS:
        ms = [v["ms"] for v in legs[leg]]
        last = legs[leg][-1]
        row["/".join(leg)] = dict(best_ms=min(ms), median_ms=statistics.median(ms), all_ms=ms, turns=last["turns"],
                                  capped=last["turns"] >= max_iter, final_residual=last["res"],
                                  basis_bytes=last["basis_bytes"],
                                  true_residual=true_residual(case, b, x_last[leg], last["norm_factor"]),
                                  us_per_turn=1e3 * statistics.median(ms) / max(1, last["turns"]))
    s2 = reg.solver("k", capi.default_config(solver=capi.SOLVER_GMRES, preconditioner=capi.PRECOND_BJ, max_block_size=1,
                                             krylov_dim=KRYLOV_DIM, tolerance=0.0, rel_tol=0.0, max_iter=2,
                                             update_init_guess=1)).set_matrix(case)
    row["kernels"] = kernel_rows(s2, case, b)
    for m in ("cgs", "cgs2"):
        d, v = row[m + "/double"], row[m + "/single"]
        row[m + "/verdict"] = verdict(d["all_ms"], v["all_ms"])
        for basis, w in (("double", d), ("single", v)):
            line = (f"{name:>8} {m:<5} {basis:<6} median {w['median_ms']:10.3f} ms (best {w['best_ms']:10.3f}; rounds "
                    f"{' '.join(f'{t:.3f}' for t in w['all_ms'])}) {w['turns']:5d} turns{' (maxIter)' if w['capped'] else ''} "
                    f"{w['us_per_turn']:9.2f} us/turn | residual {w['final_residual']:.3e} true {w['true_residual']:.3e} | "
                    f"basis {w['basis_bytes'] / 1e6:.1f} MB")
            print(line, flush=True)
            lines.append(line)
        line = (f"{name:>8} {m:<5} single against double: {row[m + '/verdict']}; solve x{d['median_ms'] / v['median_ms']:.3f}, "
                f"per turn x{d['us_per_turn'] / v['us_per_turn']:.3f}, turns {v['turns'] - d['turns']:+d}; spread of the "
                f"double legs {max(d['all_ms']) - min(d['all_ms']):.3f} ms")
        print(line, flush=True)
        lines.append(line)
    line = f"{name:>8} (the block kernels alone, 20 launches each:)"
    for kr in row["kernels"]:
        line += (f"\n{name:>8} {kr['kernel']:<10} {kr['basis']:<6} it {kr['it']:2d}: {kr['us']:9.2f} us = {kr['share']:.3f} of "
                 f"8 TB/s on {kr['bytes']:.3e} B")
    print(line, flush=True)
    lines.append(line)
    rows.append(row)
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,216")
    ap.add_argument("--asym", type=int, default=126)  # 126^3 = 2,000,376 rows
    ap.add_argument("--big", type=int, default=368)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, rows = [], []
    for n in [int(x) for x in a.sizes.split(",") if x]:
        case = synthetic.poisson_case(n)
        run(f"{n}^3", case, synthetic.rhs_for_x_star(case)[0], a.rounds, a.max_iter, lines, rows)
    if a.asym > 0:
        case = synthetic.poisson_case(a.asym, symmetric=False)
        run(f"{a.asym}^3a", case, synthetic.rhs_for_x_star(case)[0], a.rounds, a.max_iter, lines, rows)
    if a.big > 0:
        case = synthetic.poisson_case(a.big)
        run(f"{a.big}^3", case, synthetic.rhs_for_x_star(case)[0], a.rounds, a.max_iter, lines, rows)
    text = "\n".join(lines) + "\n" + json.dumps(rows) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
