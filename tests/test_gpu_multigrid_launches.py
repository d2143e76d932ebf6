"""Preconditioner Multigrid: mgLaunchesPerApply pinned absolutely.  The count is worked out from
what the solver itself reports of its hierarchy -- mgLevels, mgRows<l>, mgVisits<l>, mgTailLevels -- and the cycle's plan:
with L levels, the first t = L - mgTailLevels of them launched, nu sweeps and k iterations of the coarsest CG,

    sum over the launched levels l < t of mgVisits<l> c_l  +  mgVisits<t> if t < L (the tail: one launch per visit of its
    first level)  +  2 on a renumbered device copy (the vectors carried into the caller's order and back)

    c_0 where level 0 is the system matrix on the in-loop layout: 4 nu + 2 in double precision (a product and the sweep or
        restriction behind it: two launches; the prolongation one of its own), 2 nu + 3 in single precision (the sweep
        or the residual is the product's epilogue)
    c_l of a level with a CSR matrix of its own (level 0 of a renumbered copy, and 0 < l < L - 1): 2 nu + 1 (first
        pre-sweep, nu - 1 further ones, the restriction, nu post-sweeps with the prolongation folded into the first)
    c_{L-1} of a launched coarsest level: 1 + 7 k, and one more in single precision when L = 1 (z widened to doubles)"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (case, config): poisson_sym keeps level 0 on the in-loop layout; shuffled14 with renumber on, as
# test_gpu_multigrid.test_renumbered_equals_caller_numbering sets it up, gives level 0 a CSR copy of its own
SETUPS = {
    "poisson_sym": (base.CASES["poisson_sym"], capi.RENUMBER_OFF),
    "shuffled14": (lambda: synthetic.renumber_case(synthetic.poisson_case(14), 4096), capi.RENUMBER_ON),
}


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def expected_launches(s, nu, k, single, renumbered):
    levels = int(s.get_property("mgLevels"))
    t = levels - int(s.get_property("mgTailLevels"))
    visits = [int(s.get_property(f"mgVisits{l}")) for l in range(levels)]
    total = 0
    for l in range(t):
        if l == levels - 1:
            cost = 1 + 7 * k + (1 if single and levels == 1 else 0)
        elif l == 0 and not renumbered:
            cost = 2 * nu + 3 if single else 4 * nu + 2
        else:
            cost = 2 * nu + 1
        total += visits[l] * cost
    if t < levels:
        total += visits[t]
    return total + (2 if renumbered else 0)


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("name", sorted(SETUPS))
def test_launches_per_apply(reg, name, precision):
    make, renumber = SETUPS[name]
    case = make()
    r = base.rhs(case.n_cells)
    single, renumbered = precision == "single", renumber == capi.RENUMBER_ON

    def applied(tail, nu, gamma, k):
        mg = dict(aggregation="hashed", aggregatePasses=2, smootherSweeps=nu, coarseVisits=gamma, coarseSolverIters=k,
                  cyclePrecision=precision)
        s = base.device(reg, f"launches_{name}_{precision}", case, mg=mg, props=(("mgTailRows", tail),), renumber=renumber)
        s.apply_preconditioner(r)
        return s

    s = applied(0.0, 1, 1, 4)
    levels = int(s.get_property("mgLevels"))
    rows = [int(s.get_property(f"mgRows{l}")) for l in range(levels)]
    assert levels >= 4 and rows[0] == case.n_cells and rows[2] < 512 < rows[0], rows
    tails_seen = set()
    for tail in (0.0, float(rows[2]), 512.0):
        for nu in (1, 3):
            for gamma in (1, 2):
                for k in (4, 0):
                    s = applied(tail, nu, gamma, k)
                    assert s.get_property("renumbered") == (1.0 if renumbered else 0.0)
                    assert s.get_property("mgCyclePrecisionInUse") == (1.0 if single else 0.0)
                    assert [int(s.get_property(f"mgRows{l}")) for l in range(int(s.get_property("mgLevels")))] == rows
                    in_tail = int(s.get_property("mgTailLevels"))
                    assert in_tail == sum(1 for n in rows if n <= tail), (tail, rows)
                    got = int(s.get_property("mgLaunchesPerApply"))
                    want = expected_launches(s, nu, k, single, renumbered)
                    print(f"{name} {precision} tail {tail:.0f} ({in_tail} of {levels} levels) nu {nu} visits {gamma} "
                          f"iters {k}: launches {got}, expected {want}")
                    assert got == want, (name, precision, tail, in_tail, rows, nu, gamma, k)
                    tails_seen.add(in_tail)
    assert 0 in tails_seen and len(tails_seen) >= 2, tails_seen  # (launch by launch, and with a tail)
