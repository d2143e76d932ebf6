"""tests/mg_single_walk.py on the CPU (Multigrid's `cyclePrecision single`): run with float64 the
walk is the double references' own cycle bit for bit; the cases of tests/test_gpu_multigrid_single.py produce no binary32
subnormal; and as a preconditioner of the oracle's CG the single walk needs at most one turn more than the double one
(24^3, pgm / 1 and pgm / 3, tolerance 1e-6 and 1e-10 -- a condition, not a measurement; the counts are printed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import precond_cases as pc  # noqa: E402
import mg_single_walk as sw  # noqa: E402
from mixed_walk import TINY32  # noqa: E402
from test_gpu_multigrid import DEFAULTS, rhs  # noqa: E402
from test_gpu_multigrid_visits import VisitRef  # noqa: E402

# the cases of the GPU comparison: name -> (case, aggregation, aggregatePasses, coarseVisits)
CASES = {
    "block_10_9_7": (lambda: synthetic.poisson_block(10, 9, 7), "pgm", 1, 1),
    "poisson14": (lambda: synthetic.poisson_case(14), "pgm", 1, 1),
    "poisson14_hashed": (lambda: synthetic.poisson_case(14), "hashed", 2, 2),
    "poisson12_asym": (lambda: synthetic.poisson_case(12, symmetric=False), "pgm", 1, 1),
    "voronoi": (lambda: synthetic.voronoi_case(3000), "pgm", 1, 1),
    "periodic_x": (lambda: synthetic.poisson_block(10, 8, 6, periodic_x=True), "pgm", 1, 1),
}


def hierarchy(oracle, case, aggregation, passes, gamma):
    ref = VisitRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    return ref.with_gamma(gamma)


@pytest.mark.parametrize("name", sorted(CASES))
def test_in_float64_the_walk_is_the_double_reference(oracle, name):
    make, aggregation, passes, gamma = CASES[name]
    case = make()
    ref = hierarchy(oracle, case, aggregation, passes, gamma)
    assert ref.levels >= 3
    r = rhs(case.n_cells)
    walk = sw.SingleWalk(ref, np.float64)
    np.testing.assert_array_equal(walk.apply(r), ref.apply(r))
    assert walk.visits == ref.visits
    single = sw.SingleWalk(ref)
    z = single.apply(r)
    # (the single walk is another function of r, and a close one: binary32 carries 24 bits)
    assert not np.array_equal(z, ref.apply(r))
    assert np.abs(z - ref.apply(r)).max() <= 1e-4 * np.abs(ref.apply(r)).max()
    assert single.smallest_fp32 >= TINY32, single.smallest_fp32


def test_a_value_beyond_binary32_is_refused(oracle):
    case = synthetic.poisson_case(6)
    rp, cols, vals = oracle_csr(oracle, case)
    vals = vals.copy()
    vals[7] = 1e39
    ref = VisitRef(oracle, rp, cols, vals, **dict(DEFAULTS, aggregation="pgm", aggregatePasses=1))
    with pytest.raises(OverflowError) as e:
        sw.SingleWalk(ref)
    assert "level 0" in str(e.value)


@pytest.mark.parametrize("passes", [1, 3])
def test_single_needs_at_most_one_turn_more(oracle, passes):
    case = synthetic.poisson_case(24)
    rp, cols, vals = oracle_csr(oracle, case)
    b = np.ones(case.n_cells)
    ref = hierarchy(oracle, case, "pgm", passes, 1)
    A = oracle.DistMatrix(rp, cols, vals)
    counts = {}
    for tolerance in (1e-6, 1e-10):
        for word, walk in (("double", ref), ("single", sw.SingleWalk(ref))):
            got = pc.oracle_solve(A, b, pc.callback(walk.apply), "cg", tolerance=tolerance, max_iter=500)
            assert got.final_residual <= tolerance and got.n_iterations < 500, (word, tolerance, got.n_iterations)
            counts[word, tolerance] = got.n_iterations
    print(f"pgm / {passes}: iterations {counts}")
    for tolerance in (1e-6, 1e-10):
        assert counts["single", tolerance] <= counts["double", tolerance] + 1, counts
