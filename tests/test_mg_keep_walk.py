"""tests/mg_keep_walk.py on the CPU (Multigrid's `aggregateCaching`, DESIGN.md section 7b, "kept aggregates"), on the cases
of tests/test_gpu_multigrid.py with pgm / 1 and hashed / 3.  (a) With unchanged values the refreshed hierarchy is the full
generation's bit for bit.  (b) With every third row's diagonal scaled by 1.5 the patterns and aggregates are the record's,
a fresh generation would choose other aggregates at every level -- so the GPU comparison discriminates -- and every coarse
value is within k 2^-53 sum|terms| of the exact sum (math.fsum) of its k terms of the level above under the level's composed
map: the rounding bound of any k-term sum, whatever its association -- a condition, not a measurement."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import oracle_csr  # noqa: E402
import mg_keep_walk as kw  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
from test_gpu_multigrid import Csr, DEFAULTS  # noqa: E402
from test_gpu_multigrid_aggregation import PassRef  # noqa: E402

VARIANTS = [("pgm", 1), ("hashed", 3)]
_built = {}


def built(oracle, name, aggregation, passes):
    """(case, its matrix, full reference, record, scaled matrix), each made once."""
    key = (name, aggregation, passes)
    if key not in _built:
        case = base.CASES[name]()
        csr = oracle_csr(oracle, case)
        mg = dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes)
        full = PassRef(oracle, *csr, **mg)
        rec = kw.record(Csr(*csr), aggregation, passes, DEFAULTS["maxLevels"], DEFAULTS["minCoarseRows"])
        changed = oracle_csr(oracle, base.scaled(case, 1.5, slice(0, case.n_cells, 3)))
        _built[key] = (case, csr, full, rec, changed)
    return _built[key]


def same_pattern(A, B):
    return np.array_equal(A.rp, B.rp) and np.array_equal(A.cols, B.cols)


@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_unchanged_values_give_the_full_generation(oracle, name, aggregation, passes):
    _, csr, full, rec, _ = built(oracle, name, aggregation, passes)
    kept = kw.KeptRef(oracle, *csr, rec)
    assert kept.levels == full.levels >= 3 and kept.passes == full.passes
    assert 480 <= full.A[0].n <= 3000
    for l in range(full.levels):
        assert same_pattern(kept.A[l], full.A[l]), l
        np.testing.assert_array_equal(kept.A[l].vals, full.A[l].vals, err_msg=f"vals of level {l}")
        np.testing.assert_array_equal(kept.inv_d[l], full.inv_d[l], err_msg=f"1 / d of level {l}")
    for l in range(full.levels - 1):
        np.testing.assert_array_equal(kept.agg[l], full.agg[l], err_msg=f"agg of level {l}")
        for a, b in zip(kept.members[l], full.members[l]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_changed_values_keep_the_record_and_round_like_a_sum(oracle, name, aggregation, passes):
    _, csr, full, rec, changed = built(oracle, name, aggregation, passes)
    kept = kw.KeptRef(oracle, *changed, rec)
    fresh = PassRef(oracle, *changed, **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    assert kept.levels == full.levels
    np.testing.assert_array_equal(kept.A[0].vals, changed[2])
    assert not np.array_equal(kept.A[0].vals, full.A[0].vals)
    for l in range(full.levels):
        assert same_pattern(kept.A[l], full.A[l]), l
    worst = 0.0
    for l in range(full.levels - 1):
        np.testing.assert_array_equal(kept.agg[l], full.agg[l], err_msg=f"agg of level {l}")
        # (the premise of the GPU comparison: a generation from these values chooses other aggregates, level by level)
        assert l >= len(fresh.agg) or not np.array_equal(fresh.agg[l], kept.agg[l]), f"level {l}: the same aggregates"
        A, C, comp = kept.A[l], kept.A[l + 1], kept.agg[l]
        k = comp[A.rows] * C.n + comp[A.cols]
        order = np.argsort(k, kind="stable")
        ks, terms = k[order], A.vals[order]
        hs = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        assert len(hs) == len(C.vals)
        np.testing.assert_array_equal(ks[hs], C.rows * C.n + C.cols)
        for g, (lo, hi) in enumerate(zip(hs, np.r_[hs[1:], len(ks)])):
            t = terms[lo:hi]
            bound = (hi - lo) * 2.0 ** -53 * float(np.abs(t).sum())
            err = abs(float(C.vals[g]) - math.fsum(t))
            assert err <= bound, (l, g, err, bound)
            worst = max(worst, err / bound if bound > 0.0 else 0.0)
    print(f"{name} {aggregation}/{passes}: levels {full.levels}, largest error / bound {worst:.3f}")
