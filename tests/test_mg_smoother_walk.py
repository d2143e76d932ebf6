"""tests/mg_smoother_walk.py on the CPU (Multigrid's `smootherSweeps` and `correctionScale`): at nu = 2,
alpha = 1 the walk is VisitRef's own apply bit for bit, in float64 and through the single walk; and as the preconditioner of
the oracle's CG, one sweep with the correction scaled by 1.25 costs at most 0.8 of today's cycle, counted as turns x
(products per apply + 1), on a hierarchy of hashed / 3 -- a condition, not a measurement; the counts are printed.  The
counts on the deep hierarchies of pgm / 1 are printed and not asserted: they are the warning DESIGN carries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import precond_cases as pc  # noqa: E402
import mg_single_walk as sw  # noqa: E402
import mg_smoother_walk as smw  # noqa: E402
from test_gpu_multigrid import DEFAULTS, rhs  # noqa: E402
from test_mg_single_walk import CASES  # noqa: E402


def hierarchy(oracle, case, aggregation, passes, gamma=1):
    ref = smw.SmoothRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    return ref.with_gamma(gamma)


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_sweeps_unscaled_are_the_visit_reference(oracle, name):
    make, aggregation, passes, gamma = CASES[name]
    case = make()
    ref = hierarchy(oracle, case, aggregation, passes, gamma)
    assert ref.levels >= 3 and (ref.nu, ref.alpha) == (2, 1.0)
    r = rhs(case.n_cells)
    plain = ref.as_visit_ref()
    want = plain.apply(r)
    np.testing.assert_array_equal(ref.apply(r), want)
    assert ref.visits == plain.visits
    # (and the single walk of it is SingleWalk's own)
    np.testing.assert_array_equal(smw.SmoothSingle(ref).apply(r), sw.SingleWalk(plain).apply(r))
    np.testing.assert_array_equal(smw.SmoothSingle(ref, np.float64).apply(r), want)
    # negative control: another count or another scale is another function of r
    for nu, alpha in ((1, 1.0), (2, 1.5), (3, 1.0)):
        assert not np.array_equal(ref.with_smoother(nu, alpha).apply(r), want), (nu, alpha)


def test_products_per_apply_follow_the_sweeps(oracle):
    """2 nu products on every level but the coarsest (nu - 1 pre-sweeps with one, the residual, nu post-sweeps), and the
    coarsest CG's; a continued visit's first pre-sweep is a full one."""
    case = synthetic.poisson_case(12)
    ref = hierarchy(oracle, case, "hashed", 2)
    nnz = [len(A.cols) for A in ref.A]
    r = rhs(case.n_cells)
    for nu in (1, 2, 3, 4):
        walk = ref.with_smoother(nu, 1.0)
        walk.apply(r)
        assert walk.work == 2 * nu * sum(nnz[:-1]) + ref.iters * nnz[-1], nu
    two = ref.with_smoother(1, 1.25, gamma=2)
    two.apply(r)
    assert ref.levels >= 4 and two.visits[1] == 2
    v = two.visits
    continued = [0] + [v[l] - v[l - 1] for l in range(1, ref.levels - 1)]  # (one product more each)
    assert two.work == sum((2 * v[l] + continued[l]) * nnz[l] for l in range(ref.levels - 1)) + v[-1] * ref.iters * nnz[-1]


def turns(oracle, case, walk, max_iter=500):
    rp, cols, vals = oracle_csr(oracle, case)
    got = pc.oracle_solve(oracle.DistMatrix(rp, cols, vals), np.ones(case.n_cells), pc.callback(walk.apply), "cg",
                          tolerance=1e-6, max_iter=max_iter)
    return got.n_iterations, got.final_residual


@pytest.mark.parametrize("name", ["poisson24", "voronoi8000"])
def test_one_scaled_sweep_costs_at_most_four_fifths(oracle, name):
    """hashed / 3, b = 1, tolerance 1e-6: turns x (products per apply + 1) at nu = 1, alpha = 1.25 against nu = 2, alpha = 1.
    The reference alone gives 0.64 (24^3) and 0.47 (Voronoi 8,000)."""
    case = synthetic.poisson_case(24) if name == "poisson24" else synthetic.voronoi_case(8000)
    ref = hierarchy(oracle, case, "hashed", 3)
    cost, seen = {}, {}
    for nu, alpha in ((2, 1.0), (1, 1.25)):
        walk = ref.with_smoother(nu, alpha)
        its, res = turns(oracle, case, walk)
        assert res <= 1e-6 and its < 500, (nu, alpha, its, res)
        cost[nu, alpha] = its * (walk.products + 1.0)
        seen[nu, alpha] = (its, round(walk.products, 2))
    ratio = cost[1, 1.25] / cost[2, 1.0]
    print(f"{name} hashed / 3: (turns, products per apply) {seen}, cost ratio {ratio:.3f}")
    assert ratio <= 0.8, (ratio, seen)


def test_the_counts_on_deep_hierarchies_are_printed(oracle):
    """pgm / 1 (eight to ten levels): the scale is applied on every level, and a fixed one is sensitive there.  Printed, not
    asserted."""
    rows = [("poisson_case(24)", synthetic.poisson_case(24), [(2, 1.0), (1, 1.0), (1, 1.25)]),
            ("poisson_block(20,16,12)", synthetic.poisson_block(20, 16, 12), [(2, 1.0), (1, 1.5)]),
            ("voronoi_case(8000)", synthetic.voronoi_case(8000), [(2, 1.0), (2, 1.5)])]
    for name, case, variants in rows:
        ref = hierarchy(oracle, case, "pgm", 1)
        for nu, alpha in variants:
            walk = ref.with_smoother(nu, alpha)
            its, res = turns(oracle, case, walk)
            print(f"{name} pgm / 1 ({ref.levels} levels) nu {nu} alpha {alpha}: {its} turns, residual {res:.2e}, "
                  f"{walk.products:.2f} products per apply")
