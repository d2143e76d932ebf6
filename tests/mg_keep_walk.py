"""The contract of Multigrid's `aggregateCaching` ("kept aggregates") as a NumPy walk: the record of
a full generation -- per kept level the coarse indices of each of its passes -- and the hierarchy a refresh makes of new
values under that record.  Every pass sums the entries of ITS source matrix (the pass before it, rounded) in ascending
(row, stored position) order from the first term: the passes are not composed.  The aggregation is `coarsen` of
tests/test_gpu_multigrid_aggregation.py, the cycle is Ref's.  Shared by tests/test_mg_keep_walk.py (CPU) and
tests/test_gpu_multigrid_keep.py."""
import numpy as np

from test_gpu_multigrid import Csr, diagonal, seq_sums
from test_gpu_multigrid_aggregation import PassRef, coarsen


def record(A0, aggregation, passes, maxLevels, minCoarseRows):
    """Per kept level the list of its passes' coarse indices, as PassRef's loop chooses them on A0."""
    rec, A = [], A0
    while len(rec) < maxLevels and A.n > minCoarseRows:
        level = []
        for _ in range(passes):
            got = coarsen(A, aggregation)
            if got is None:  # (dropped: it ends the level's passes)
                break
            level.append(got[0])
            A = got[1]
            if A.n <= minCoarseRows:
                break
        if not level:
            break
        rec.append(level)
    return rec


def galerkin(A, cidx):
    """The coarse matrix of A under the coarse indices cidx: the second half of `coarsen`."""
    nc = int(cidx.max()) + 1
    k = cidx[A.rows] * nc + cidx[A.cols]
    order = np.argsort(k, kind="stable")  # ascending (i, stored position) within every (I, J)
    ks = k[order]
    hs = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cv = seq_sums(hs, np.diff(np.r_[hs, len(ks)]), A.vals[order])
    cr, cc = ks[hs] // nc, ks[hs] % nc
    rp = np.concatenate([[0], np.cumsum(np.bincount(cr, minlength=nc))])
    return Csr(rp, cc, cv)


def refresh(B0, rec):
    """The matrices of the hierarchy of B0 whose every pass takes the recorded coarse indices."""
    mats = [B0]
    for level in rec:
        A = mats[-1]
        for cidx in level:
            A = galerkin(A, cidx)
        mats.append(A)
    return mats


class KeptRef(PassRef):
    """The hierarchy a refresh leaves: matrices refresh(B0, rec), agg / members / passes those of the record, 1 / d of its
    own matrices.  The V-cycle is Ref's."""

    def __init__(self, oracle, rowptr, cols, vals, rec, coarseSolverIters=4):
        self.oracle, self.iters = oracle, coarseSolverIters
        self.A = refresh(Csr(rowptr, cols, vals), rec)
        self.agg, self.passes = [], [len(level) for level in rec]
        for level in rec:
            comp = level[0]
            for cidx in level[1:]:
                comp = cidx[comp]
            self.agg.append(comp)
        self.inv_d = [1.0 / diagonal(A) for A in self.A]
        self.members = []
        for agg, A in zip(self.agg, self.A[1:]):
            order = np.argsort(agg, kind="stable")
            self.members.append((order, np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=A.n))])))
