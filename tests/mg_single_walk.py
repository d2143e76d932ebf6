"""The contract of Multigrid's `cyclePrecision single` ("the cycle in single precision") as a NumPy
walk: the apply of the coarse-visits cycle with binary32 operands and binary32 operations on a hierarchy that was
generated in float64.  Every product and every sum is one NumPy operation of the walk's type (rounded once), every
quotient is formed in float64 and rounded once, the coarsest CG's sums are the oracle's reductions on the float64 casts
(mixed_walk's wide sums) in the device's tree (helpers.blocked, as the double reference's CG).  The walk is built on a
reference of the double cycle (Ref / PassRef / VisitRef of the GPU test modules) and shares its hierarchy; run with float64 it is
that reference's own cycle.  Shared by tests/test_mg_single_walk.py (CPU) and tests/test_gpu_multigrid_single.py."""
import numpy as np

from ogl_amd import capi
from helpers import blocked
from mixed_walk import Tracker

F32, F64 = np.float32, np.float64
OMEGA = 0.9  # (rounded to the walk's type: fl32(0.9) in single)


def row_sums(starts, lens, terms, dtype, track=None):
    """out[g] = ((0 + t[s]) + t[s + 1]) + ... over the run [starts[g], starts[g] + lens[g]) of `terms`, every sum one
    operation of `dtype`."""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    acc = np.zeros(len(starts), dtype)
    for t in range(int(lens.max()) if len(lens) else 0):
        m = t < lens
        acc[m] = acc[m] + terms[starts[m] + t]
        if track is not None:
            track(acc[m])
    return acc


class SingleWalk:
    """The cycle of `ref` (its hierarchy, coarseSolverIters and -- unless given -- its coarse visits) in `dtype`."""

    def __init__(self, ref, dtype=F32, gamma=None):
        self.ref, self.T = ref, dtype
        self.gamma = gamma if gamma is not None else getattr(ref, "gamma", 1)
        self.track = Tracker() if dtype == F32 else None
        self.levels = ref.levels
        self.omega = dtype(OMEGA)
        self.vals = [self.rounded(A.vals, f"a coefficient of level {l}") for l, A in enumerate(ref.A)]
        self.inv_d = [self.rounded(d, f"the inverse diagonal of level {l}") for l, d in enumerate(ref.inv_d)]

    def rounded(self, v, what):
        v = np.asarray(v, F64)
        with np.errstate(over="ignore"):
            out = v.astype(self.T)
        bad = np.flatnonzero(np.isfinite(v) & ~np.isfinite(out))
        if bad.size:
            raise OverflowError(f"{what} is finite in double precision and not in single precision (position {bad[0]})")
        return self.seen(out)

    def seen(self, v):
        return v if self.track is None else self.track(v)

    @property
    def smallest_fp32(self):
        return np.inf if self.track is None else self.track.smallest

    def mul(self, A, vals, x):
        """(A x)_i from 0 in ascending stored column order, products and sums of the walk's type."""
        return row_sums(A.rp[:-1], np.diff(A.rp), self.seen(vals * x[A.cols]), self.T, self.track)

    def sweep(self, l, A, vals, b, x):
        s = self.mul(A, vals, x)
        return self.seen(x + self.seen(self.omega * self.seen(self.seen(b - s) * self.inv_d[l])))

    def wide(self, u, v):
        return self.ref.oracle.dot(u.astype(F64), v.astype(F64))

    def cg(self, A, vals, b):
        T = self.T
        x, r, p = np.zeros(A.n, T), b.copy(), np.zeros(A.n, T)
        rho = 0.0
        with blocked(self.ref.oracle, capi.lib().ogl_reduction_chunk_rows()):
            for it in range(self.ref.iters):
                prev = 1.0 if it == 0 else rho
                rho = self.wide(r, r)
                tmp = T(0.0 if prev == 0.0 else rho / prev)
                p = self.seen(r + self.seen(tmp * p))
                q = self.mul(A, vals, p)
                beta = self.wide(p, q)
                if beta != 0.0:
                    t = T(rho / beta)
                    x = self.seen(x + self.seen(t * p))
                    r = self.seen(r - self.seen(t * q))
        return x

    def cycle(self, l, b, fine=None, x=None):
        ref = self.ref
        if l == 0:
            self.visits = [0] * self.levels
        self.visits[l] += 1
        A, vals = ref.A[l], self.vals[l]
        if l == 0 and fine is not None:
            A, vals = fine, self.rounded(fine.vals, "a coefficient of level 0")
        if l == self.levels - 1:
            return self.cg(A, vals, b)
        if x is None:
            x = self.sweep(l, A, vals, b, self.seen(self.omega * self.seen(b * self.inv_d[l])))
        else:
            x = self.sweep(l, A, vals, b, self.sweep(l, A, vals, b, x))
        res = self.seen(b - self.mul(A, vals, x))
        order, ptr = ref.members[l]
        bc = row_sums(ptr[:-1], np.diff(ptr), res[order], self.T, self.track)
        xc = self.cycle(l + 1, bc)
        if l + 1 < self.levels - 1:
            for _ in range(self.gamma - 1):
                xc = self.cycle(l + 1, bc, x=xc)
        x = self.seen(x + xc[ref.agg[l]])
        x = self.sweep(l, A, vals, b, x)
        return self.sweep(l, A, vals, b, x)

    def apply(self, r, fine=None):
        """z = (double) x of the cycle on b = fl(r); fine: the matrix whose products the fine level takes."""
        b = self.seen(np.asarray(r, F64).astype(self.T))
        return self.cycle(0, b, fine).astype(F64)
