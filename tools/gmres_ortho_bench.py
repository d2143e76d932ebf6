"""The Gram-Schmidt step of GKOGMRES (property orthoMethod: mgs | cgs | cgs2) under GKOGMRES(30) + BJ(1) on one GPU: the
three methods in alternation on the same box and the same solver handle, after a warm-up solve of each; every solve starts
from x = 0 (updateInitGuess 1) and runs to tolerance 1e-6 (relTol 0) or --max-iter, whichever comes first.  The mgs legs of
the same run are the baseline.

    python tools/gmres_ortho_bench.py [--sizes 100,216] [--asym 126] [--big 368] [--rounds 5] [--big-rounds 1]
                                      [--max-iter 2000] [--out profiles/<file>.txt]

Per case and method: solve time (t_solve_ms: the loop, device events and a synchronise at its end; best and median of the
rounds), turns, microseconds per turn, the recorded residual and the true one (sum |b - A x| / norm factor, formed on the
host from the LDU arrays), launches per turn.  Per case: every kernel of the block form alone (property
orthoTimedLaunches: HIP events around back-to-back launches on the solve's own buffers) at columns it = 0, 15 and 29 with
its share of 8 TB/s on the bytes its model moves from and to HBM, k = it + 1 basis vectors: multidot 8 N (k + 1), the
update 8 N (k + 2) -- with cgs2's second-round partials ("UpdateDots") a thread holds its rows of V in registers for up to 32
basis vectors, so the bytes are the same -- and the finaliser's 8 k n_chunks."""
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
METHODS = ("mgs", "cgs", "cgs2")
KRYLOV_DIM = 30


def true_residual(case, b, x, norm_factor):
    return float(np.sum(np.abs(b - synthetic.apply_case(case, x)))) / norm_factor


def kernel_rows(s, case, b):
    """The new kernels alone, after a short cgs2 solve that leaves the buffers of the block form behind."""
    n = case.n_cells
    nc = -(-n // capi.lib().ogl_reduction_chunk_rows())
    s.set_ortho_method("cgs2")
    s.set_property("orthoTimedLaunches", 20.0)
    s.solve(b, np.zeros_like(b))
    s.set_property("orthoTimedLaunches", 0.0)
    out = []
    for it in (0, 15, 29):
        k = it + 1
        for key, bytes_moved in (("orthoMultidotUs", 8.0 * n * (k + 1)), ("orthoFinHUs", 8.0 * k * nc),
                                 ("orthoUpdateUs", 8.0 * n * (k + 2)), ("orthoUpdateDotsUs", 8.0 * n * (k + 2))):
            us = s.get_property(f"{key}_{it}")
            out.append(dict(kernel=key[5:-2], it=it, us=us, bytes=bytes_moved, share=bytes_moved / (us * 1e-6) / PEAK))
    return out


def run(name, case, b, rounds, max_iter, lines, rows):
    reg = capi.Registry()
    s = reg.solver("p", capi.default_config(solver=capi.SOLVER_GMRES, preconditioner=capi.PRECOND_BJ, max_block_size=1,
                                            krylov_dim=KRYLOV_DIM, tolerance=1e-6, rel_tol=0.0, max_iter=max_iter,
                                            update_init_guess=1))
    s.set_matrix(case)
    legs = {m: [] for m in METHODS}
    x_last, folded = {}, 0.0
    for rnd in range(rounds + 1):  # round 0 warms every method up
        for m in METHODS:
            s.set_ortho_method(m)
            x, perf = s.solve(b, np.zeros_like(b))
            assert s.get_property("orthoMethodInUse") == capi.ORTHO_METHOD[m]
            if m == "mgs":
                folded = s.get_property("fusedFinalizersInUse")
            if rnd:
                legs[m].append(dict(ms=perf.t_solve_ms, turns=perf.n_iterations - 1, res=perf.final_residual,
                                    norm_factor=perf.norm_factor, launches=s.get_property("gmresLaunchesPerTurn")))
                x_last[m] = x
            print(f"# {name} round {rnd} {m}: {perf.t_solve_ms:.3f} ms, {perf.n_iterations - 1} turns", flush=True)
    row = dict(case=name, rows=case.n_cells, krylov_dim=KRYLOV_DIM, max_iter=max_iter)
    for m in METHODS:
        ms = [leg["ms"] for leg in legs[m]]
        last = legs[m][-1]
        row[m] = dict(best_ms=min(ms), median_ms=statistics.median(ms), all_ms=ms, turns=last["turns"],
                      capped=last["turns"] >= max_iter, final_residual=last["res"], launches_per_turn=last["launches"],
                      true_residual=true_residual(case, b, x_last[m], last["norm_factor"]),
                      us_per_turn=1e3 * min(ms) / max(1, last["turns"]))
    # (the kernels alone: a solve of two turns is enough to own the buffers)
    s2 = reg.solver("k", capi.default_config(solver=capi.SOLVER_GMRES, preconditioner=capi.PRECOND_BJ, max_block_size=1,
                                             krylov_dim=KRYLOV_DIM, tolerance=0.0, rel_tol=0.0, max_iter=2,
                                             update_init_guess=1)).set_matrix(case)
    row["kernels"] = kernel_rows(s2, case, b)
    rows.append(row)
    base = row["mgs"]
    for m in METHODS:
        v = row[m]
        line = (f"{name:>8} {m:<5} {v['best_ms']:10.3f} ms (median {v['median_ms']:10.3f}) {v['turns']:5d} turns"
                f"{' (maxIter)' if v['capped'] else ''} {v['us_per_turn']:9.2f} us/turn x{base['us_per_turn'] / v['us_per_turn']:.3f}"
                f" | {v['launches_per_turn']:.1f} launches/turn | residual {v['final_residual']:.3e} true {v['true_residual']:.3e}"
                f" | solve x{base['best_ms'] / v['best_ms']:.3f}")
        print(line, flush=True)
        lines.append(line)
    line = f"{name:>8} (mgs with {'folded links' if folded else 'a finaliser launch per link'}; the kernels of the block form alone:)"
    for kr in row["kernels"]:
        line += (f"\n{name:>8} {kr['kernel']:<10} it {kr['it']:2d}: {kr['us']:9.2f} us = {kr['share']:.3f} of 8 TB/s on "
                 f"{kr['bytes']:.3e} B")
    print(line, flush=True)
    lines.append(line)
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,216")
    ap.add_argument("--asym", type=int, default=126)  # 126^3 = 2,000,376 rows
    ap.add_argument("--big", type=int, default=368)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-rounds", type=int, default=1)
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
        run(f"{a.big}^3", case, synthetic.rhs_for_x_star(case)[0], a.big_rounds, a.max_iter, lines, rows)
    text = "\n".join(lines) + "\n" + json.dumps(rows) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
