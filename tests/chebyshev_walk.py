"""The contract of preconditioner Chebyshev as a Python/NumPy walk, every line one rounded double
operation:

* bound: lambda_max = max_i (sum_j |a_ij|, stored order, from 0) / |a_ii| -- the Gershgorin bound of D^-1 A;
* coefficients: the table c0, a_k, b_k of the recurrence for [lambda_max / ratio, lambda_max], on float64 scalars (Python's
  floats with IEEE division: x / 0 without an exception);
* apply: z = p(D^-1 A) D^-1 r -- z1 = (r w) c0, then per step t = r - A z through oracle.spmv_adv (from r_i, every rounded
  product subtracted in ascending column order), t = w t, t = b_k t, u = z - z_prev, u = a_k u, z_next = (z + u) + t.

Shared by tests/test_chebyshev_walk.py (CPU), tests/test_gpu_chebyshev.py and tests/chebyshev_ranks_worker.py (GPU).  Walk
wraps one local matrix; Walk.precond() is the oracle.CallbackPrecond that makes the oracle's own cg / bicgstab / gmres
the whole-solve references."""
import math

import numpy as np

MAX_DEGREE = 16
DEFAULT_DEGREE, DEFAULT_RATIO = 4, 30.0


def bound(rowptr, cols, vals):
    """The computed lambda_max; a quotient that is not finite (a zero or missing diagonal) counts as +inf."""
    rowptr, cols = np.asarray(rowptr), np.asarray(cols)
    vals = [float(v) for v in np.asarray(vals, np.float64)]
    best = 0.0
    for i in range(len(rowptr) - 1):
        s, d = 0.0, None
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            s = s + abs(vals[e])
            if d is None and int(cols[e]) == i:
                d = vals[e]
        d = abs(0.0 if d is None else d)
        with np.errstate(all="ignore"):
            q = float(np.float64(s) / np.float64(d))
        if not math.isfinite(q):
            q = math.inf
        best = max(best, q)
    return best


class Table:
    """lambda_max, lambda_min, c0 and a[k - 1], b[k - 1] of step k = 1 .. degree."""

    def __init__(self, lambda_max, ratio, degree):
        assert 1 <= degree <= MAX_DEGREE
        self.lambda_max, self.degree = float(lambda_max), degree
        self.breakdown = not (self.lambda_max > 0.0 and math.isfinite(self.lambda_max))
        with np.errstate(all="ignore"):
            lmax, ratio = np.float64(lambda_max), np.float64(ratio)
            lmin = lmax / ratio
            theta = (lmax + lmin) / np.float64(2.0)
            delta = (lmax - lmin) / np.float64(2.0)
            sigma = theta / delta
            self.lambda_min = float(lmin)
            self.c0 = float(np.float64(1.0) / theta)
            rho_prev = np.float64(1.0) / sigma
            self.a, self.b = [], []
            for _ in range(degree):
                rho = np.float64(1.0) / (np.float64(2.0) * sigma - rho_prev)
                self.a.append(float(rho * rho_prev))
                self.b.append(float((np.float64(2.0) * rho) / delta))
                rho_prev = rho


def coefficients(lambda_max, ratio=DEFAULT_RATIO, degree=DEFAULT_DEGREE):
    return Table(lambda_max, ratio, degree)


def apply(oracle, rowptr, cols, vals, w, table, r):
    r = np.ascontiguousarray(r, np.float64)
    with np.errstate(all="ignore"):
        z_prev = np.zeros_like(r)
        z = (r * w) * table.c0
        for k in range(table.degree):
            t = oracle.spmv_adv(rowptr, cols, vals, -1.0, z, 1.0, r)
            t = w * t
            t = table.b[k] * t
            u = z - z_prev
            u = table.a[k] * u
            z_prev, z = z, (z + u) + t
    return z


class Walk:
    """The preconditioner of one local matrix (rowptr, cols, vals: columns ascending per row).  lambda_max > 0 replaces the
    computed bound."""

    def __init__(self, oracle, rowptr, cols, vals, degree=DEFAULT_DEGREE, ratio=DEFAULT_RATIO, lambda_max=0.0):
        self.oracle = oracle
        self.csr = (np.asarray(rowptr), np.asarray(cols), np.asarray(vals, np.float64))
        with np.errstate(all="ignore"):
            self.w = oracle.jacobi_generate_scalar(*self.csr)
        self.bound = lambda_max if lambda_max > 0.0 else bound(*self.csr)
        self.table = Table(self.bound, ratio, degree)

    def apply(self, r):
        return apply(self.oracle, *self.csr, self.w, self.table, r)

    def on_matrix(self, rowptr, cols, vals):
        """This object -- its w and its table as they are -- applied with another matrix in the products: a stored
        preconditioner (keyword caching) in a later time step."""
        import copy
        other = copy.copy(self)
        other.csr = (np.asarray(rowptr), np.asarray(cols), np.asarray(vals, np.float64))
        return other

    def precond(self):
        return self.oracle.CallbackPrecond(self.apply)

    def polynomial(self, lam):
        """q(lambda) with M^-1 = q(D^-1 A) D^-1, by the same recurrence on scalars (the CPU checks)."""
        t = self.table
        lam = np.asarray(lam, np.float64)
        z_prev, z = np.zeros_like(lam), np.full_like(lam, t.c0)
        for k in range(t.degree):
            z_prev, z = z, z + t.a[k] * (z - z_prev) + t.b[k] * (1.0 - lam * z)
        return z
