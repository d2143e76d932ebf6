"""The contract of Multigrid's `smootherSweeps` and `correctionScale` ("sweeps and correction scale") as
NumPy walks: `SmoothRef` is VisitRef of tests/test_gpu_multigrid_visits.py and `SmoothSingle` is SingleWalk of
tests/mg_single_walk.py, each with only `cycle` overridden -- nu sweeps before and after the coarse correction on every
level (the first pre-sweep of a visit from nothing is omega (b inv_d), no product) and the correction added as
t = x + alpha x_c[agg], the product rounded once and then the sum.  Hierarchy, sweep, sums and the coarsest CG are the
parents' own.  Both count `work`, the matrix non-zeros the products of the last apply went over.  Shared by
tests/test_mg_smoother_walk.py (CPU) and tests/test_gpu_multigrid_smoother.py."""
import copy

import numpy as np

import mg_single_walk as sw
from test_gpu_multigrid import OMEGA, seq_sums
from test_gpu_multigrid_visits import VisitRef


class SmoothRef(VisitRef):
    """VisitRef with `nu` sweeps before and after the coarse correction and the correction scaled by `alpha`."""
    nu, alpha = 2, 1.0

    def cycle(self, l, b, fine=None, x=None):
        if l == 0:
            self.visits = [0] * self.levels
            self.work = 0
        self.visits[l] += 1
        A = fine if (l == 0 and fine is not None) else self.A[l]
        nnz = len(A.cols)
        if l == self.levels - 1:
            self.work += self.iters * nnz
            return self.cg(A, b)
        full = self.nu
        if x is None:  # (counts as the first of the nu pre-sweeps)
            x = OMEGA * (b * self.inv_d[l])
            full -= 1
        for _ in range(full):
            x = self.sweep(l, b, x, A)
        res = b - A.mul(x)
        self.work += (full + 1) * nnz
        order, ptr = self.members[l]
        bc = seq_sums(ptr[:-1], np.diff(ptr), res[order], init=np.zeros(len(ptr) - 1))
        xc = self.cycle(l + 1, bc)
        if l + 1 < self.levels - 1:
            for _ in range(self.gamma - 1):
                xc = self.cycle(l + 1, bc, x=xc)
        x = x + np.float64(self.alpha) * xc[self.agg[l]]
        for _ in range(self.nu):
            x = self.sweep(l, b, x, A)
        self.work += self.nu * nnz
        return x

    def with_smoother(self, nu, alpha, gamma=None):
        """The same hierarchy (shared, not copied) walked with these sweeps and this scale."""
        other = copy.copy(self)
        other.nu, other.alpha = nu, alpha
        if gamma is not None:
            other.gamma = gamma
        return other

    def as_visit_ref(self):
        """The same hierarchy under the imported reference's own cycle."""
        other = copy.copy(self)
        other.__class__ = VisitRef
        return other

    @property
    def products(self):
        """Products of the last apply in fine-level non-zeros."""
        return self.work / len(self.A[0].cols)


class SmoothSingle(sw.SingleWalk):
    """SingleWalk of a SmoothRef with the same override: nu, alpha and gamma are the reference's; the scale is fl(alpha) in
    the walk's type and t = x + fl(alpha) x_c[agg] is formed in it, each operation rounded once."""

    def __init__(self, ref, dtype=sw.F32):
        super().__init__(ref, dtype)
        self.nu, self.alpha = ref.nu, dtype(ref.alpha)

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
        full = self.nu
        if x is None:
            x = self.seen(self.omega * self.seen(b * self.inv_d[l]))
            full -= 1
        for _ in range(full):
            x = self.sweep(l, A, vals, b, x)
        res = self.seen(b - self.mul(A, vals, x))
        order, ptr = ref.members[l]
        bc = sw.row_sums(ptr[:-1], np.diff(ptr), res[order], self.T, self.track)
        xc = self.cycle(l + 1, bc)
        if l + 1 < self.levels - 1:
            for _ in range(self.gamma - 1):
                xc = self.cycle(l + 1, bc, x=xc)
        x = self.seen(x + self.seen(self.alpha * xc[ref.agg[l]]))
        for _ in range(self.nu):
            x = self.sweep(l, A, vals, b, x)
        return x
