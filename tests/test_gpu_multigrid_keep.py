"""Preconditioner Multigrid with `aggregateCaching N` ("kept aggregates") against the NumPy walk of
tests/mg_keep_walk.py: a refreshed hierarchy keeps the aggregates and patterns of the object's last full generation and
carries the CURRENT values, bit for bit what a full generation would make of them under those aggregates -- matrices,
1 / d (through the apply) and z = M^-1 r.  One field with caching 0 generates the registry's stored object on its first
solve and its own object afterwards, each with a record of its own: full, full, refresh, refresh, full, ..."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import mg_keep_walk as kw  # noqa: E402
import mg_single_walk as sw  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
import test_gpu_multigrid_aggregation as agg  # noqa: E402
from test_gpu_multigrid import Csr  # noqa: E402
from test_gpu_multigrid_aggregation import PassRef  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = base.DEFAULTS
VARIANTS = [("pgm", 1), ("hashed", 3)]
_kept = {}


def third_rows(case, factor):
    return base.scaled(case, factor, slice(0, case.n_cells, 3))


def fresh_ref(oracle, case, aggregation, passes, **mg):
    return PassRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes, **mg))


def kept_ref(oracle, made_for, now, aggregation, passes, **mg):
    """The hierarchy of `now`'s values under the aggregates a full generation chooses on `made_for`."""
    p = dict(DEFAULTS, **mg)
    rec = kw.record(Csr(*oracle_csr(oracle, made_for)), aggregation, passes, p["maxLevels"], p["minCoarseRows"])
    return kw.KeptRef(oracle, *oracle_csr(oracle, now), rec, coarseSolverIters=p["coarseSolverIters"])


def changed_of(oracle, name, aggregation, passes):
    """(case, changed case, KeptRef of the changed values under the case's aggregates, fresh PassRef of the changed case),
    each built once."""
    key = (name, aggregation, passes)
    if key not in _kept:
        case = agg.case_of(name)
        changed = third_rows(case, 1.5)
        _kept[key] = (case, changed, kept_ref(oracle, case, changed, aggregation, passes),
                      fresh_ref(oracle, changed, aggregation, passes))
    return _kept[key]


def solve(reg, name, case, aggregation, passes, keep=2, mg=None, **kw_):
    mg = dict(mg or {})
    if keep is not None:
        mg["aggregateCaching"] = keep
    return agg.device(reg, name, case, aggregation, passes, mg=mg, **kw_)


def refreshed(reg, name, first, third, aggregation, passes, **kw_):
    """Three solves of the first field of a registry: the stored object in full, the own object in full (both on `first`),
    the own object refreshed with the values of `third`."""
    for case in (first, first):
        s = solve(reg, name, case, aggregation, passes, **kw_)
        assert s.get_property("mgAggregatesReused") == 0.0 and s.get_property("mgGenerateHostReads") > 0.0
    s = solve(reg, name, third, aggregation, passes, **kw_)
    assert s.get_property("mgAggregatesReused") == 1.0 and s.get_property("mgGenerateHostReads") == 0.0
    # (the maps: one int32 per source entry and per coarse entry of every pass at the least; none on a single level)
    assert (s.get_property("mgKeptBytes") > 0.0) == (s.get_property("mgLevels") > 1.0)
    return s


def assert_kept(s, kept, fresh, r, apply=None):
    """The device holds `kept` -- and not `fresh`, whose aggregates are asserted to differ at every level."""
    for l in range(kept.levels - 1):
        assert l >= len(fresh.agg) or not np.array_equal(fresh.agg[l], kept.agg[l]), f"level {l}: the same aggregates"
    agg.assert_hierarchy(s, kept)
    np.testing.assert_array_equal(s.apply_preconditioner(r), (apply or kept.apply)(r))


@pytest.fixture()
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module", autouse=True)
def _forget():
    yield
    _kept.clear()


# ---- 1. same values ----
@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_same_values_reproduce_the_full_generation(oracle, reg, name, aggregation, passes):
    case, ref = agg.ref_of(oracle, name, aggregation, passes)
    s = refreshed(reg, "same", case, case, aggregation, passes)
    agg.assert_hierarchy(s, ref)
    r = base.rhs(case.n_cells)
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))


# ---- 2. changed values ----
@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_changed_values_under_kept_aggregates(oracle, reg, name, aggregation, passes):
    case, changed, kept, fresh = changed_of(oracle, name, aggregation, passes)
    s = refreshed(reg, "changed", case, changed, aggregation, passes)
    assert_kept(s, kept, fresh, base.rhs(case.n_cells))


# ---- 3. the counter ----
def test_counter_full_full_refresh_refresh(oracle, reg):
    case = synthetic.poisson_case(10)
    r = base.rhs(case.n_cells)
    steps = [third_rows(case, 1.0 + 0.5 * t) for t in range(7)]
    reused, left = [], []
    for t, made_for in enumerate((0, 1, 1, 1, 4, 4, 4)):
        s = solve(reg, "counter", steps[t], "hashed", 3)
        reused.append(s.get_property("mgAggregatesReused"))
        left.append(s.get_property("mgAggregateCachingLeft"))
        assert (s.get_property("mgGenerateHostReads") == 0.0) == (reused[-1] == 1.0)
        kept = kept_ref(oracle, steps[made_for], steps[t], "hashed", 3)
        if t != made_for:
            assert_kept(s, kept, fresh_ref(oracle, steps[t], "hashed", 3), r)
        else:
            agg.assert_hierarchy(s, fresh_ref(oracle, steps[t], "hashed", 3))
            agg.assert_hierarchy(s, kept)
    assert reused == [0, 0, 1, 1, 0, 1, 1], reused
    assert left == [2, 2, 1, 0, 2, 1, 0], left


# ---- 4. under caching ----
def test_with_caching_the_own_object_is_refreshed(oracle, reg):
    """caching 2, aggregateCaching 5: solves 1, 2, 4 and 5 apply the stored hierarchy of step 0 as it is; solve 3 generates
    the own object in full, solve 6 refreshes it."""
    case = synthetic.poisson_case(10)
    r = base.rhs(case.n_cells)
    steps = [third_rows(case, 1.0 + 0.5 * t) for t in range(7)]
    refs = [fresh_ref(oracle, c, "hashed", 3) for c in steps]
    for t in range(7):
        s = solve(reg, "cached", steps[t], "hashed", 3, keep=5, caching=2)
        if t in (0, 3):
            assert s.get_property("mgAggregatesReused") == 0.0 and s.get_property("mgGenerateHostReads") > 0.0
            agg.assert_hierarchy(s, refs[t])
            np.testing.assert_array_equal(s.apply_preconditioner(r), refs[t].apply(r))
        elif t == 6:
            assert s.get_property("mgAggregatesReused") == 1.0 and s.get_property("mgGenerateHostReads") == 0.0
            assert_kept(s, kept_ref(oracle, steps[3], steps[6], "hashed", 3), refs[6], r)
        else:
            assert s.get_property("mgAggregatesReused") == 0.0
            np.testing.assert_array_equal(s.mg_level(0)[3], refs[0].agg[0], err_msg=f"step {t}")
            np.testing.assert_array_equal(s.apply_preconditioner(r), refs[0].apply(r, fine=refs[t].A[0]), err_msg=f"step {t}")
    assert not np.array_equal(refs[3].agg[0], refs[0].agg[0]) and not np.array_equal(refs[6].agg[0], refs[3].agg[0])


# ---- 5. invalidation ----
@pytest.mark.parametrize("what", ["pattern", "aggregatePasses", "aggregation", "minCoarseRows", "aggregateCaching0"])
def test_invalidation(oracle, reg, what):
    case = agg.case_of("poisson_sym")
    s = refreshed(reg, "inval", case, case, "pgm", 1)
    kept_bytes = s.get_property("mgKeptBytes")
    new, variant, mg, keep = third_rows(case, 1.5), ("pgm", 1), {}, 2
    if what == "pattern":
        new = synthetic.poisson_block(10, 8, 6)
    elif what == "aggregatePasses":
        variant = ("pgm", 3)
    elif what == "aggregation":
        variant = ("hashed", 1)
    elif what == "minCoarseRows":
        mg = dict(minCoarseRows=40)
    else:
        keep = 0
    s = solve(reg, "inval", new, *variant, keep=keep, mg=mg)
    assert s.get_property("mgAggregatesReused") == 0.0 and s.get_property("mgGenerateHostReads") > 0.0
    ref = fresh_ref(oracle, new, *variant, **mg)
    agg.assert_hierarchy(s, ref)
    r = base.rhs(new.n_cells)
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))
    if what == "aggregateCaching0":  # (the maps may stay; nothing is reused, now or at the next solve)
        assert s.get_property("mgKeptBytes") in (0.0, kept_bytes) and s.get_property("mgAggregateCachingLeft") == 0.0
        s = solve(reg, "inval", case, *variant, keep=0)
        assert s.get_property("mgAggregatesReused") == 0.0
        agg.assert_hierarchy(s, agg.ref_of(oracle, "poisson_sym", "pgm", 1)[1])


# ---- 6. the renumbered device copy and the layouts ----
def test_renumbered_device_copy(oracle, reg):
    """Level 0 is the caller-numbered copy: its values are gathered through map0 again, then refreshed like any other."""
    case = synthetic.renumber_case(synthetic.poisson_case(14), 4096)
    changed = third_rows(case, 1.5)
    s = refreshed(reg, "rn", case, changed, "hashed", 3, renumber=capi.RENUMBER_ON)
    assert s.get_property("renumbered") == 1.0
    assert_kept(s, kept_ref(oracle, case, changed, "hashed", 3), fresh_ref(oracle, changed, "hashed", 3),
                base.rhs(case.n_cells))


@pytest.mark.parametrize("layout", sorted(base.LAYOUTS))
def test_every_layout(oracle, reg, layout):
    case, changed, kept, fresh = changed_of(oracle, "poisson_sym", "hashed", 3)
    cfg, (lay, half) = base.LAYOUTS[layout]
    s = refreshed(reg, "lay_" + layout, case, changed, "hashed", 3, props=(("streamAboveBytes", 0.0),), **cfg)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert_kept(s, kept, fresh, base.rhs(case.n_cells))


# ---- 7. cyclePrecision single ----
def test_single_precision_twin_is_rounded_again(oracle, reg):
    case, changed, kept, fresh = changed_of(oracle, "poisson_sym", "hashed", 3)
    s = refreshed(reg, "single", case, changed, "hashed", 3, mg=dict(cyclePrecision="single"))
    assert s.get_property("mgCyclePrecisionInUse") == 1.0
    r = base.rhs(case.n_cells)
    stale = sw.SingleWalk(agg.ref_of(oracle, "poisson_sym", "hashed", 3)[1]).apply(r, fine=kept.A[0])
    want = sw.SingleWalk(kept).apply(r)
    assert not np.array_equal(stale, want)  # (the twin of the generation before would show)
    assert_kept(s, kept, fresh, r, apply=lambda v: want)


# ---- 8. edges ----
@pytest.mark.parametrize("aggregation", ["hashed", "pgm"])
@pytest.mark.parametrize("what", ["diagonal", "two_rows", "maxLevels1"])
def test_edges(oracle, reg, what, aggregation):
    mg = {}
    if what == "diagonal":  # one level: a refresh is 1 / d alone
        line = synthetic.poisson_block(40, 1, 1)
        none = np.zeros(0, np.int32)
        case = synthetic.LduCase(40, none, none, line.diag, np.zeros(0), None, [], line.global_index, 40)
        levels = 1
    elif what == "two_rows":
        case, mg, levels = synthetic.poisson_block(2, 1, 1), dict(minCoarseRows=0), 2
    else:
        case, mg, levels = synthetic.poisson_case(12), dict(maxLevels=1), 2
    changed = third_rows(case, 1.5)
    r = base.rhs(case.n_cells)
    kept = kept_ref(oracle, case, changed, aggregation, 3, **mg)
    assert kept.levels == levels
    s = refreshed(reg, f"edge_{what}", case, changed, aggregation, 3, mg=mg)
    agg.assert_hierarchy(s, kept)
    np.testing.assert_array_equal(s.apply_preconditioner(r), kept.apply(r))


# ---- 9. refusals and the default ----
@pytest.mark.parametrize("value", [-1, 0.5])
def test_refusals(reg, value):
    case = synthetic.poisson_case(6)
    s = reg.solver("keep_refuse", base.cfg()).set_multigrid(aggregateCaching=value).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == capi.ERR_INVALID and "aggregateCaching" in str(e.value), e.value
    s.set_multigrid(aggregateCaching=1)
    _, perf = s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert perf.n_iterations > 0


def test_default_keeps_nothing(oracle, reg):
    case, ref = agg.ref_of(oracle, "poisson_sym", "hashed", 3)
    for _ in range(3):
        s = solve(reg, "default", case, "hashed", 3, keep=None)
        assert s.get_property("mgAggregatesReused") == 0.0 and s.get_property("mgKeptBytes") == 0.0
        assert s.get_property("mgGenerateHostReads") > 0.0 and s.get_property("mgAggregateCachingLeft") == 0.0
    agg.assert_hierarchy(s, ref)


# ---- 10. the ledger ----
def test_time_steps_allocate_nothing_after_the_second_full_generation():
    """Ten time steps that alternate between two coefficient sets: the own object is generated in full at steps 1, 4 and 7;
    from step 4 on the ledger stands still, and nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    sets = [case, third_rows(case, 1.5)]
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks, reused = {}, []
    for step in range(10):
        s = reg.solver("keep_steps", base.cfg()).set_multigrid(aggregation="hashed", aggregatePasses=3, aggregateCaching=2)
        s.set_matrix(sets[step % 2]).solve(b, np.zeros_like(b))
        reused.append(s.get_property("mgAggregatesReused"))
        if step in (4, 9):
            marks[step] = capi.memory_ledger().as_dict()
            assert s.get_property("mgKeptBytes") > 0.0
    reg.close()
    assert reused == [0, 0, 1, 1, 0, 1, 1, 0, 1, 1], reused
    for k in soak_worker.LEDGER_EXACT:
        assert marks[9][k] == marks[4][k], (k, marks)
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
