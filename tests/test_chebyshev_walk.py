"""What the walk of preconditioner Chebyshev (tests/chebyshev_walk.py) must satisfy to pin anything, on the CPU: under the
oracle's own loops it cuts GKOCG's checks to at most 0.4 of scalar Jacobi's and lets GKOGMRES(10) stop on the criterion,
its polynomial is positive on the spectrum of D^-1 A, its bound is one, and a forced lambda_max is taken."""
import functools

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr
import chebyshev_walk as cw

BOXES = {"6x6x6": (6, 6, 6), "10x9x7": (10, 9, 7), "12x12x12": (12, 12, 12)}
CRIT = dict(tolerance=1e-8, rel_tol=0.0, max_iter=2000)


@functools.lru_cache(maxsize=None)
def system(name):
    from oracle import oracle
    oracle.build()
    case = synthetic.poisson_block(*BOXES[name])
    return oracle, oracle_csr(oracle, case), synthetic.rhs_for_x_star(case)[0]


@functools.lru_cache(maxsize=None)
def solve(name, solver, degree):
    """The oracle's solve in the device's reduction tree; degree 0: scalar Jacobi.  Computed once; do not change it."""
    oracle, csr, b = system(name)
    P = cw.Walk(oracle, *csr, degree=degree).precond() if degree else oracle.jacobi_generate_scalar(*csr)
    A = oracle.DistMatrix(*csr)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        if solver == "gmres":
            return oracle.gmres(A, b, np.zeros_like(b), P, krylov_dim=10, **CRIT)
        return oracle.cg(A, b, np.zeros_like(b), P, **CRIT)


@pytest.mark.parametrize("name", list(BOXES))
def test_cg_takes_at_most_four_tenths_of_jacobis_checks(name):
    jac, cheb = solve(name, "cg", 0), solve(name, "cg", 4)
    print(name, "GKOCG checks: BJ(1)", jac.n_iterations, "degree 4", cheb.n_iterations)
    assert jac.final_residual < 1e-8 and cheb.final_residual < 1e-8
    assert cheb.n_iterations <= 0.4 * jac.n_iterations, (cheb.n_iterations, jac.n_iterations)


@pytest.mark.parametrize("name", list(BOXES))
def test_gmres10_stops_on_the_criterion(name):
    ref = solve(name, "gmres", 4)
    print(name, "GKOGMRES(10) checks, degree 4:", ref.n_iterations)
    assert ref.final_residual < 1e-8 and ref.n_iterations <= CRIT["max_iter"], (ref.n_iterations, ref.final_residual)


def _spectrum(name):
    oracle, (rp, cols, vals), _ = system(name)
    n = len(rp) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), cols] = vals
    d = np.diag(A)
    # D^-1 A is similar to the symmetric D^-1/2 A D^-1/2
    return np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d)))


def test_the_bound_is_an_upper_bound_of_the_spectrum():
    oracle, csr, _ = system("6x6x6")
    lam = _spectrum("6x6x6")
    assert lam.min() > 0.0
    assert cw.bound(*csr) >= lam.max(), (cw.bound(*csr), lam.max())


@pytest.mark.parametrize("degree", range(1, 9))
def test_the_polynomial_is_positive_on_the_spectrum(degree):
    oracle, csr, _ = system("6x6x6")
    w = cw.Walk(oracle, *csr, degree=degree)
    q = w.polynomial(_spectrum("6x6x6"))
    assert (q > 0.0).all(), q.min()
    # ... and on all of (0, lambda_max], which is what keeps M positive definite whatever the spectrum is
    assert (w.polynomial(np.linspace(1e-9, w.bound, 4001)) > 0.0).all()


def test_the_polynomial_is_the_apply():
    """polynomial() is apply() on the eigenvalues: M^-1 = D^-1/2 V q(Lambda) V^T D^-1/2 with D^-1/2 A D^-1/2 = V Lambda V^T."""
    oracle, (rp, cols, vals), _ = system("6x6x6")
    n = len(rp) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), cols] = vals
    h = 1.0 / np.sqrt(np.diag(A))
    lam, V = np.linalg.eigh(A * np.outer(h, h))
    w = cw.Walk(oracle, rp, cols, vals, degree=5)
    r = np.random.default_rng(1).standard_normal(n)
    want = h * (V @ (w.polynomial(lam) * (V.T @ (h * r))))
    np.testing.assert_allclose(w.apply(r), want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_a_forced_lambda_max_makes_the_table_of_that_value():
    oracle, csr, _ = system("6x6x6")
    w = cw.Walk(oracle, *csr, degree=3, ratio=10.0, lambda_max=1.75)
    t, want = w.table, cw.coefficients(1.75, 10.0, 3)
    assert (t.lambda_max, t.lambda_min, t.c0, t.a, t.b) == (1.75, 0.175, want.c0, want.a, want.b)
    theta, delta = (1.75 + 0.175) / 2.0, (1.75 - 0.175) / 2.0
    assert t.c0 == 1.0 / theta
    rho0 = 1.0 / (theta / delta)
    rho1 = 1.0 / (2.0 * (theta / delta) - rho0)
    assert t.a[0] == rho1 * rho0 and t.b[0] == (2.0 * rho1) / delta
    assert not t.breakdown and cw.coefficients(float("inf")).breakdown and cw.coefficients(0.0).breakdown


def test_a_zero_diagonal_breaks_the_bound():
    oracle, (rp, cols, vals), _ = system("6x6x6")
    vals = np.array(vals, np.float64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    vals[np.flatnonzero((rows == 5) & (np.asarray(cols) == 5))[0]] = 0.0
    assert cw.bound(rp, cols, vals) == float("inf")
    assert cw.Walk(oracle, rp, cols, vals).table.breakdown
