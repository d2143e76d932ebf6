"""The keyword guessProjectionCredit as a walk composed from guess_projection_walk.project and the
oracle's solvers, without a solver loop of its own.  With the credit the criterion's initial normalised residual is
init_res = S0 / norm_factor -- S0 = sum |b - A x0| at the CALLER's guess, which the pre-step forms; norm_factor the solve's
own, formed at the projected guess -- and nothing else of the solve changes.  So the credited solve with (tolerance T,
relTol R) is the plain solve from the projected guess with tolerance max(T, R * init_res) and relTol 0: res < T or
res < R * init_res is res < max(T, R * init_res) at every check, the first one included.  A probe at max_iter 0 gives the
norm factor; division and product are one rounded float64 operation each.  Shared by
tests/test_guess_projection_credit_walk.py (CPU) and tests/test_gpu_guess_projection_credit.py."""
import math

import numpy as np

import guess_projection_walk as pw

SEQ_TOLERANCE = pw.SEQ_CRITERION["tolerance"]


def credit_applies(p):
    """Whether a projection (guess_projection_walk.project) is credited: vectors were offered, a column was kept (else x
    is still the caller's guess and the solve is the plain one) and S0 is finite and > 0."""
    return p.offered >= 1 and p.kept >= 1 and math.isfinite(p.norm_before) and p.norm_before > 0.0


def credited_threshold(p, norm_factor, tolerance, rel_tol):
    """(init_res, the tolerance of the equivalent plain solve): one IEEE division, one rounded product."""
    init_res = float(np.float64(p.norm_before) / np.float64(norm_factor))
    return init_res, max(float(tolerance), float(np.float64(rel_tol) * np.float64(init_res)))


def credited_solve(p, solve, tolerance, rel_tol):
    """The solve after the pre-step p with the credit on.  solve(guess, tolerance=, rel_tol=, max_iter=None) -> an oracle
    Result (max_iter None: the caller's own).  Returns (result, credited); a credited result reports the credited initial
    residual, everything else is the equivalent plain solve's."""
    if not credit_applies(p):
        return solve(p.x, tolerance=tolerance, rel_tol=rel_tol), False
    probe = solve(p.x, tolerance=tolerance, rel_tol=rel_tol, max_iter=0)
    init_res, thr = credited_threshold(p, probe.norm_factor, tolerance, rel_tol)
    res = solve(p.x, tolerance=thr, rel_tol=0.0)
    assert res.norm_factor == probe.norm_factor
    res.initial_residual = init_res
    return res, True


def run_sequence(oracle, K, steps, csr_of, rel_tol, credit, tolerance=SEQ_TOLERANCE):
    """guess_projection_walk.run_sequence under a relTol: credit is a bool or a function of the step number (the keyword
    switched between steps on one handle).  Returns a list of (projection, result, ring as a list of vectors, credited)."""
    ring, out = pw.Ring(K), []
    x = np.zeros(pw.SEQ_SHAPE[0] * pw.SEQ_SHAPE[1] * pw.SEQ_SHAPE[2])
    for n in range(steps):
        case = pw.sequence_case(n)
        rp, cols, vals = csr_of(case)
        b = pw.sequence_rhs(case, n)
        A = oracle.DistMatrix(rp, cols, vals)
        inv = oracle.jacobi_generate_scalar(rp, cols, vals)
        on = credit(n) if callable(credit) else bool(credit)

        def cg(guess, tolerance, rel_tol, max_iter=None):
            return oracle.cg(A, b, guess, inv, tolerance=tolerance, rel_tol=rel_tol,
                             max_iter=1000 if max_iter is None else max_iter)

        # (the post-step is guess_projection_walk.step's: the whole step x_final - x0 when a column was kept or a turn ran)
        p = pw.project(oracle, rp, cols, vals, b, x, ring.vectors if ring.K else [])
        res, credited = credited_solve(p, cg, tolerance, rel_tol) if on else (cg(p.x, tolerance, rel_tol), False)
        if ring.K and (p.kept >= 1 or res.n_iterations >= 2):
            ring.store(res.x - x)
        p.stored = len(ring.vectors)
        out.append((p, res, [v.copy() for v in ring.vectors], credited))
        x = res.x
    return out


# ---- the rings of the single-solve tests: steps that nearly contain the error of the caller's guess ----

def x_star_of(rp, cols, vals, b):
    """The solution of a small system by a dense solve (the tests' boxes have at most 1,728 rows)."""
    n = len(rp) - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(A, (rows, np.asarray(cols)), np.asarray(vals))
    return np.linalg.solve(A, b)


def credit_ring(x_star, x0, k, c_range, seed=11):
    """d_j = c_j (x* - x0) + 0.05 |x* - x0|_inf u_j, c_j uniform in c_range, u_j uniform in (-1, 1)^n: the projection takes
    most of the error of the caller's guess out, as the steps of a time loop do, and leaves the noise -- the larger the c_j
    the less of it."""
    rng = np.random.default_rng(seed)
    e = np.asarray(x_star) - np.asarray(x0)
    amp = 0.05 * np.abs(e).max()
    return [c * e + amp * rng.uniform(-1, 1, e.size) for c in rng.uniform(c_range[0], c_range[1], k)]


# The single solves of tests/test_gpu_guess_projection_credit.py: the system (tests/test_gpu_guess_projection.py: system), the
# oracle's solver and the range of the c_j, chosen per system so that the projection lowers sum |r| at least five times and
# the credited solve ends at least two checks before the one without the credit (tests/test_guess_projection_credit_walk.py
# holds both).  GKOGMRES looks at the residual of its last restart: with krylovDim 10 its checks can end a solve at counts
# 1, 12, 23, ... only, and one cycle already gives the factor 100 of relTol 0.01 -- so its ring is the one that meets the
# credited criterion at the first check.
SINGLE_TOLERANCE, SINGLE_REL_TOL, SINGLE_K = 1e-8, 0.01, 4
SINGLE = {
    "GKOCG_none": ("10x9x7", "cg_none", (2.0, 6.0)),
    "GKOCG_BJ1_half": ("12x12x12", "cg_bj", (1.0, 3.0)),
    "GKOCG_BJ1_csr": ("12x12x12", "cg_bj", (1.0, 3.0)),
    "GKOBiCGStab_BJ1": ("random", "bicgstab_bj", (0.5, 1.5)),
    "GKOGMRES10": ("9x9x7", "gmres10_bj", (40.0, 80.0)),
    "renumber_on": ("12x12x12", "cg_bj", (1.0, 3.0)),
}


def single_ring(what, csr, b, x0):
    return credit_ring(x_star_of(*csr, b), x0, SINGLE_K, SINGLE[what][2])


# The solves that end at their first check: the ring holds x* - x0 alone, so the projected guess is x* up to rounding and its
# normalised residual is near 1e-15 -- below any tolerance one would set, which would end the solve with or without the
# credit.  So these run with tolerance 0: relTol alone decides.  Credited, it is met at the first check; as built it asks
# for a hundredth of the rounding-level residual and the solve goes on -- FIRST_CHECK_BUILT_MAX_ITER bounds that run.
FIRST_CHECK = ("GKOCG_BJ1_half", "GKOBiCGStab_BJ1", "GKOGMRES10")
FIRST_CHECK_TOLERANCE, FIRST_CHECK_BUILT_MAX_ITER = 0.0, 3
