"""The keyword guessProjectionCredit on the CPU: what the oracle alone says about the inputs of
tests/test_gpu_guess_projection_credit.py.  Under relTol the keyword guessProjection as built costs checks on the time-step
sequence of tests/guess_projection_walk.py -- relTol is measured from the residual at the projected guess --; counted from
the caller's guess it saves them.  The credited solve is composed in tests/guess_projection_credit_walk.py from the
existing walk of the pre-step and the oracle's solvers."""
import numpy as np
import pytest

from helpers import blocked, oracle_csr
import guess_projection_walk as pw
import guess_projection_credit_walk as cw
import test_gpu_guess_projection as base

CHUNK_ROWS = 512
REL_TOL = 0.05


@pytest.fixture(scope="module")
def sequences(oracle):
    """The ten steps at relTol 0.05: K = 0, K = 4 as built, K = 4 credited; computed once."""
    with blocked(oracle, CHUNK_ROWS):
        return {key: cw.run_sequence(oracle, K, 10, lambda c: oracle_csr(oracle, c), REL_TOL, credit)
                for key, (K, credit) in {"K0": (0, False), "built": (4, False), "credited": (4, True)}.items()}


def counts(seq):
    return [res.n_iterations for _, res, _, _ in seq]


def test_credited_sequence_has_the_recorded_counts(sequences):
    """Checks per step, tolerance 1e-9, relTol 0.05, blocked sums with chunk 512."""
    its = {key: counts(seq) for key, seq in sequences.items()}
    print(its)
    assert its["K0"] == [18, 5, 6, 8, 8, 11, 10, 7, 7, 6]
    assert its["built"] == [18, 5, 13, 12, 30, 30, 30, 26, 26, 16]  # the keyword as built costs checks under relTol
    assert its["credited"] == [18, 5, 3, 7, 3, 7, 7, 2, 1, 5]
    assert [c for *_, c in sequences["credited"]] == [False] + [True] * 9  # step 1 has nothing to project on
    assert not any(c for *_, c in sequences["built"])


def test_credited_sequence_saves_checks_over_k0(sequences):
    its = {key: counts(seq) for key, seq in sequences.items()}
    assert (sum(its["credited"][2:]), sum(its["K0"][2:])) == (35, 63)
    assert sum(its["credited"][2:]) < sum(its["K0"][2:]) < sum(its["built"][2:])


def test_credited_sequence_has_a_solve_that_ends_at_its_first_check(sequences):
    """A projection that already meets relTol from the caller's guess: no turn, and the stored step is the projection's."""
    hits = [(p, res, ring) for p, res, ring, _ in sequences["credited"] if res.n_iterations == 1]
    assert hits
    for p, res, ring in hits:
        np.testing.assert_array_equal(res.x, p.x)
        assert p.kept >= 1 and res.final_residual < REL_TOL * res.initial_residual


def test_credited_solve_is_the_plain_one_where_nothing_is_credited(oracle):
    """An empty ring, and a ring of zero vectors (every column dropped: the guess stays the caller's)."""
    _, _, (rp, cols, vals), b, x0, _ = base.system(oracle, "10x9x7")
    A = oracle.DistMatrix(rp, cols, vals)

    def cg(guess, tolerance, rel_tol, max_iter=None):
        return oracle.cg(A, b, guess, None, tolerance=tolerance, rel_tol=rel_tol, max_iter=300 if max_iter is None else max_iter)

    with blocked(oracle, CHUNK_ROWS):
        plain = cg(x0, 1e-8, 0.01)
        for ring in ([], [np.zeros_like(b)] * 3):
            p = pw.project(oracle, rp, cols, vals, b, x0, ring)
            res, credited = cw.credited_solve(p, cg, 1e-8, 0.01)
            assert not credited and p.kept == 0
            np.testing.assert_array_equal(res.history, plain.history)
            np.testing.assert_array_equal(res.x, plain.x)
            assert res.initial_residual == plain.initial_residual


def oracle_solver(oracle, kind, csr, b):
    rp, cols, vals = csr
    A = oracle.DistMatrix(rp, cols, vals)
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    if kind == "gmres10_bj":
        P = oracle.Precond(rp, cols, vals, 1)
        return lambda g, tolerance, rel_tol, max_iter=None: oracle.gmres(
            A, b, g, P, tolerance=tolerance, rel_tol=rel_tol, max_iter=300 if max_iter is None else max_iter, krylov_dim=10)
    fn, d = {"cg_none": (oracle.cg, None), "cg_bj": (oracle.cg, inv), "bicgstab_bj": (oracle.bicgstab, inv)}[kind]
    return lambda g, tolerance, rel_tol, max_iter=None: fn(
        A, b, g, d, tolerance=tolerance, rel_tol=rel_tol, max_iter=300 if max_iter is None else max_iter)


@pytest.mark.parametrize("what", cw.FIRST_CHECK)
def test_first_check_inputs_stop_by_the_credit_alone(oracle, what):
    """The ring that holds x* - x0: at the tests' usual tolerance the solve ends at its first check with or without the
    credit (the projected guess is x* up to rounding), which would show nothing; at tolerance 0 the credited solve ends
    there and the solve as built goes on."""
    name, kind, _ = cw.SINGLE[what]
    _, _, csr, b, x0, _ = base.system(oracle, name)
    solve = oracle_solver(oracle, kind, csr, b)
    rp, cols, vals = csr
    with blocked(oracle, CHUNK_ROWS):
        p = pw.project(oracle, rp, cols, vals, b, x0, [cw.x_star_of(*csr, b) - x0])
        usual = solve(p.x, tolerance=cw.SINGLE_TOLERANCE, rel_tol=cw.SINGLE_REL_TOL)
        built = solve(p.x, tolerance=cw.FIRST_CHECK_TOLERANCE, rel_tol=cw.SINGLE_REL_TOL,
                      max_iter=cw.FIRST_CHECK_BUILT_MAX_ITER)
        credited, on = cw.credited_solve(p, solve, cw.FIRST_CHECK_TOLERANCE, cw.SINGLE_REL_TOL)
    print(f"{what}: checks at tolerance {cw.SINGLE_TOLERANCE} {usual.n_iterations}; at tolerance 0 as built "
          f"{built.n_iterations}, credited {credited.n_iterations}")
    assert on and p.kept == 1
    assert usual.n_iterations == 1 and usual.initial_residual < cw.SINGLE_TOLERANCE
    assert credited.n_iterations == 1 and len(credited.history) == 1
    assert credited.final_residual < cw.SINGLE_REL_TOL * credited.initial_residual
    np.testing.assert_array_equal(credited.x, p.x)
    assert built.n_iterations > 1 and built.initial_residual == credited.final_residual


@pytest.mark.parametrize("what", list(cw.SINGLE))
def test_single_solve_inputs_show_the_credit(oracle, what):
    """Every single-solve input of the GPU file: the projection lowers sum |r| at least five times, and the credited solve
    ends at least two checks before the solve as built (the same solve with relTol counted from the projected guess)."""
    name, kind, _ = cw.SINGLE[what]
    _, _, csr, b, x0, _ = base.system(oracle, name)
    ring = cw.single_ring(what, csr, b, x0)
    solve = oracle_solver(oracle, kind, csr, b)
    rp, cols, vals = csr
    with blocked(oracle, CHUNK_ROWS):
        p = pw.project(oracle, rp, cols, vals, b, x0, ring)
        after = oracle.norm1(oracle.spmv_adv(np.asarray(rp, np.int32), np.asarray(cols, np.int32), vals, -1.0, p.x, 1.0, b))
        built = solve(p.x, tolerance=cw.SINGLE_TOLERANCE, rel_tol=cw.SINGLE_REL_TOL)
        credited, on = cw.credited_solve(p, solve, cw.SINGLE_TOLERANCE, cw.SINGLE_REL_TOL)
    print(f"{what}: S0 / sum|r| after = {p.norm_before / after:.2f}, checks as built {built.n_iterations}, "
          f"credited {credited.n_iterations}")
    assert on and p.kept == cw.SINGLE_K
    assert p.norm_before / after >= 5.0
    assert credited.n_iterations <= built.n_iterations - 2
    assert credited.initial_residual == p.norm_before / credited.norm_factor
