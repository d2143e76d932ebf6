"""Preconditioner Multigrid with `coarseVisits g` ("coarse visits"): every level below the fine one,
the coarsest excepted, is visited g times per visit of its parent -- the first visit from nothing, the others continued from
the answer before with the same right-hand side and two full pre-sweeps.  The reference is `PassRef` of
tests/test_gpu_multigrid_aggregation.py with only `cycle` overridden to that contract (hierarchy, sums and coarsest CG are
imported unchanged); it counts its visits per level.  z = M^-1 r bit for bit wherever the single-workgroup tail starts,
whole solves against the oracle's loop with the walk called back as its preconditioner, the refusals and the guard on the
number of level visits."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import precond_cases as pc  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
import test_gpu_multigrid_aggregation as aggmod  # noqa: E402
import test_gpu_precond_solves as solves  # noqa: E402
from test_gpu_multigrid import OMEGA, seq_sums  # noqa: E402
from test_gpu_multigrid_aggregation import PassRef  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = base.DEFAULTS
MAX_VISITS = 4096  # the guard: level visits of one apply, summed over the levels
# (aggregation, aggregatePasses, coarseVisits); pgm / 1 has 8 to 10 levels: 3 visits would be thousands in the walk
VARIANTS = [("hashed", 2, 2), ("hashed", 2, 3), ("hashed", 3, 2), ("pgm", 1, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
class VisitRef(PassRef):
    """PassRef whose cycle visits every level below level 0, the coarsest excepted, `gamma` times per visit of its parent;
    visits[l]: the visits of level l in the last apply."""
    gamma = 1

    def cycle(self, l, b, fine=None, x=None):
        if l == 0:
            self.visits = [0] * self.levels
        self.visits[l] += 1
        A = fine if (l == 0 and fine is not None) else self.A[l]
        if l == self.levels - 1:
            return self.cg(A, b)
        if x is None:
            x = self.sweep(l, b, OMEGA * (b * self.inv_d[l]), A)
        else:
            x = self.sweep(l, b, self.sweep(l, b, x, A), A)
        res = b - A.mul(x)
        order, ptr = self.members[l]
        bc = seq_sums(ptr[:-1], np.diff(ptr), res[order], init=np.zeros(len(ptr) - 1))
        xc = self.cycle(l + 1, bc)
        if l + 1 < self.levels - 1:
            for _ in range(self.gamma - 1):
                xc = self.cycle(l + 1, bc, x=xc)
        x = x + xc[self.agg[l]]
        x = self.sweep(l, b, x, A)
        return self.sweep(l, b, x, A)

    def with_gamma(self, gamma):
        """The same hierarchy (shared, not copied) walked with `gamma` visits."""
        other = copy.copy(self)
        other.gamma = gamma
        return other


def visits_of(levels, gamma):
    """The contract's visit counts: 1, gamma, gamma^2, ... down the levels, the coarsest as often as its parent."""
    v = [gamma ** l for l in range(levels)]
    if levels > 1:
        v[-1] = v[-2]
    return v


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
def device(reg, name, case, aggregation, passes, gamma, mg=None, props=(), **kw):
    mg = dict(mg or {})
    if gamma is not None:
        mg["coarseVisits"] = gamma
    return aggmod.device(reg, name, case, aggregation, passes, mg=mg, props=props, **kw)


_refs = {}


def ref_of(oracle, name, aggregation, passes, gamma, **mg):
    """(case, reference) of a named case; every hierarchy is built once and shared by its gammas."""
    key = (name, aggregation, passes, tuple(sorted(mg.items())))
    if key not in _refs:
        _refs[key] = VisitRef(oracle, *oracle_csr(oracle, aggmod.case_of(name)),
                              **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes, **mg))
    return aggmod.case_of(name), _refs[key].with_gamma(gamma)


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _refs.clear()


def assert_visits(s, ref):
    assert ref.visits == visits_of(ref.levels, ref.gamma), (ref.visits, ref.gamma)
    assert sum(ref.visits) <= 520, ref.visits  # (the walks of this file stay small)
    for l, v in enumerate(ref.visits):
        assert s.get_property(f"mgVisits{l}") == v, (l, ref.visits)
    assert s.get_property("coarseVisits") == ref.gamma


# ---- 1. the apply ----
@pytest.mark.parametrize("aggregation,passes,gamma", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_apply_bit_identical(oracle, reg, name, aggregation, passes, gamma):
    """z = M^-1 r for coarseSolverIters 4 and 0 (default tail), and the visits of every level."""
    for iters in (4, 0):
        case, ref = ref_of(oracle, name, aggregation, passes, gamma, coarseSolverIters=iters)
        if (aggregation, passes) == ("hashed", 2):
            assert ref.levels >= 4, ref.levels  # (a level below level 1 is really revisited)
        assert ref.levels >= 3
        r = base.rhs(case.n_cells)
        want = ref.apply(r)
        s = device(reg, f"v_{name}", case, aggregation, passes, gamma, mg=dict(coarseSolverIters=iters))
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{name} iters {iters}")
        assert_visits(s, ref)


# ---- 2. where the tail starts ----
@pytest.mark.parametrize("gamma", [2, 3])
def test_apply_bit_identical_wherever_the_tail_starts(oracle, reg, gamma):
    """mgTailRows 0 (no tail), the rows of the last level (the coarsest alone, one launch per visit of its parent), of
    level 2 (the tail's first level continued from a guess by the host), of level 1 (the recursion inside the kernel) and
    n + 1 (one launch)."""
    case, ref = ref_of(oracle, "poisson_sym", "hashed", 2, gamma)
    rows = [A.n for A in ref.A]
    assert ref.levels >= 4 and len(set(rows)) == len(rows), rows
    r = base.rhs(case.n_cells)
    want = ref.apply(r)
    launches = {}
    for tail in (0.0, float(rows[-1]), float(rows[2]), float(rows[1]), float(case.n_cells + 1)):
        for g in (gamma, 1):
            s = device(reg, "vt", case, "hashed", 2, g, props=(("mgTailRows", tail),))
            z = s.apply_preconditioner(r)
            launches[tail, g] = s.get_property("mgLaunchesPerApply")
            assert s.get_property("mgTailLevels") == sum(1 for n in rows if n <= tail), tail
            if g == 1:
                continue
            np.testing.assert_array_equal(z, want, err_msg=f"tail {tail}")
            assert_visits(s, ref)
    print("launches per apply", launches)
    assert launches[float(case.n_cells + 1), gamma] == 1
    assert launches[float(rows[1]), gamma] == launches[float(rows[1]), 1] + gamma - 1, launches
    # (the coarsest alone: one more launch per further visit of its parent, and the parent's own launches with them)
    assert launches[float(rows[-1]), gamma] > launches[float(rows[-1]), 1]
    assert launches[0.0, gamma] > launches[float(rows[-1]), gamma]


# ---- 3. every fine-level layout ----
@pytest.mark.parametrize("layout", sorted(base.LAYOUTS))
def test_apply_bit_identical_on_every_layout(oracle, reg, layout):
    """Level 0 is visited once, but its result feeds the revisited levels."""
    case, ref = ref_of(oracle, "poisson_sym", "hashed", 2, 2)
    r = base.rhs(case.n_cells)
    kw, (lay, half) = base.LAYOUTS[layout]
    s = device(reg, "vlay_" + layout, case, "hashed", 2, 2, props=(("streamAboveBytes", 0.0),), **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))


# ---- 4. one visit and the default ----
def test_one_visit_is_the_v_cycle_and_the_default(oracle, reg):
    case, ref = ref_of(oracle, "poisson_sym", "hashed", 2, 1)
    r = base.rhs(case.n_cells)
    plain = copy.copy(ref)
    plain.__class__ = PassRef  # (the same hierarchy under the imported reference's own V-cycle)
    want = plain.apply(r)
    np.testing.assert_array_equal(ref.apply(r), want)
    for gamma in (None, 1):
        s = device(reg, f"v_default_{gamma}", case, "hashed", 2, gamma)
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"coarseVisits {gamma}")
        assert s.get_property("coarseVisits") == 1
        assert [s.get_property(f"mgVisits{l}") for l in range(ref.levels)] == [1] * ref.levels


# ---- 5. negative control ----
def test_two_visits_differ_from_one(oracle, reg):
    case, two = ref_of(oracle, "poisson_sym", "hashed", 2, 2)
    one = two.with_gamma(1)
    r = base.rhs(case.n_cells)
    z1, z2 = one.apply(r), two.apply(r)
    assert not np.array_equal(z1, z2)
    z = device(reg, "v_neg", case, "hashed", 2, 2).apply_preconditioner(r)
    np.testing.assert_array_equal(z, z2)
    assert not np.array_equal(z, z1)


# ---- 6. whole solves ----
@pytest.mark.parametrize("name,solver,aggregation,passes,gamma,renumber", [
    ("sym", "cg", "hashed", 3, 2, capi.RENUMBER_OFF), ("asym", "bicgstab", "hashed", 2, 2, capi.RENUMBER_OFF),
    ("sym", "gmres", "hashed", 2, 3, capi.RENUMBER_OFF), ("shuffled14", "cg", "hashed", 3, 2, capi.RENUMBER_ON)],
    ids=lambda v: str(v))
def test_whole_solves_are_the_oracles(oracle, reg, name, solver, aggregation, passes, gamma, renumber):
    props = (("aggregation", float(capi.MG_AGGREGATION[aggregation])), ("aggregatePasses", float(passes)),
             ("coarseVisits", float(gamma)))
    got = solves.device_solve(reg, f"vws_{name}_{solver}", name, "MG", solver, props=props, renumber=renumber)
    s = got[0]
    new_id = None
    if renumber == capi.RENUMBER_ON:
        new_id = s.renumbering()
        assert new_id is not None and s.get_property("renumbered") == 1.0
        assert not np.array_equal(new_id, np.arange(new_id.size))
    key = ("whole", name, aggregation, passes)
    if key not in _refs:
        _refs[key] = VisitRef(oracle, *pc.system(name)[3], **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    walk = _refs.setdefault(key + (gamma,), _refs[key].with_gamma(gamma))  # (one object: the reference is computed once)
    assert s.get_property("coarseVisits") == gamma and walk.levels >= 3
    ref = pc.reference(name, "MG", solver, new_id=new_id, apply=walk.apply)
    # (the reference pins something: it stops by the tolerance, before max_iter, at the solution)
    assert ref.final_residual <= pc.TOL and 3 <= ref.n_iterations < pc.MAX_ITER, (ref.n_iterations, ref.final_residual)
    assert np.abs(ref.x - pc.system(name)[2]).max() <= 1e-6
    solves.assert_is_the_oracles(got, ref, solver)


# ---- 7. it preconditions ----
def walk_iterations(oracle, case, b, walk):
    rp, cols, vals = oracle_csr(oracle, case)
    ref = pc.oracle_solve(oracle.DistMatrix(rp, cols, vals), b, pc.callback(walk.apply), "cg", tolerance=1e-6, max_iter=2000)
    return ref.n_iterations


def test_two_visits_cut_the_iterations_by_a_quarter(oracle, reg):
    """poisson_case(24), hashed / 3, b = 1, GKOCG to 1e-6: strictly fewer iterations with two visits than with one and at
    most 3/4 of them; the device's counts are the walk's under the oracle's own criterion (21 and 14 iterations; under a
    plain 1-norm criterion the walk gives 20 and 13)."""
    case = synthetic.poisson_case(24)
    b = np.ones(case.n_cells)
    hierarchy = VisitRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation="hashed", aggregatePasses=3))
    its, walk = {}, {}
    for gamma in (1, 2):
        walk[gamma] = walk_iterations(oracle, case, b, hierarchy.with_gamma(gamma))
        c = capi.default_config(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_MULTIGRID, tolerance=1e-6, rel_tol=0.0,
                                max_iter=2000, renumber=capi.RENUMBER_OFF)
        s = reg.solver(f"v_it_{gamma}", c).set_multigrid(aggregation="hashed", aggregatePasses=3, coarseVisits=gamma)
        _, perf = s.set_matrix(case).solve(b, np.zeros_like(b))
        its[gamma] = perf.n_iterations
    print("iterations: device", its, "walk", walk)
    assert walk[2] < walk[1] and 4 * walk[2] <= 3 * walk[1], walk
    assert its == walk, (its, walk)
    assert its[2] < its[1] and 4 * its[2] <= 3 * its[1], its


# ---- 8. refusals and the guard ----
@pytest.mark.parametrize("value", [0, 4, 1.5])
def test_refusals(reg, value):
    case = synthetic.poisson_case(6)
    s = reg.solver(f"v_refuse_{value}", base.cfg()).set_multigrid(coarseVisits=value).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == capi.ERR_INVALID and "coarseVisits" in str(e.value), e.value


def test_too_many_visits_are_refused(oracle, reg):
    """A line of 4,000 cells with pgm / 1 and maxLevels 14: ten levels or more, thousands of visits at coarseVisits 3."""
    case = synthetic.poisson_block(4000, 1, 1)
    mg = dict(DEFAULTS, maxLevels=14)
    ref = PassRef(oracle, *oracle_csr(oracle, case), **dict(mg, aggregation="pgm", aggregatePasses=1))
    assert sum(visits_of(ref.levels, 3)) > MAX_VISITS, (ref.levels, visits_of(ref.levels, 3))
    assert sum(visits_of(ref.levels, 1)) == ref.levels
    b = np.ones(case.n_cells)
    s = reg.solver("v_guard", base.cfg()).set_multigrid(aggregation="pgm", aggregatePasses=1, coarseVisits=3, **mg)
    s.set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, np.zeros_like(b))
    assert e.value.status == capi.ERR_UNSUPPORTED and "coarseVisits" in str(e.value), e.value
    assert str(sum(visits_of(ref.levels, 3))) in str(e.value) and "aggregatePasses" in str(e.value), e.value
    s = reg.solver("v_guard", base.cfg()).set_multigrid(coarseVisits=1)
    x, perf = s.set_matrix(case).solve(b, np.zeros_like(b))
    assert s.get_property("mgLevels") == ref.levels and s.get_property("coarseVisits") == 1
    assert 0 < perf.n_iterations < 2000 and perf.final_residual <= 1e-8, (perf.n_iterations, perf.final_residual)


# ---- 9. the stored hierarchy and memory ----
def test_a_stored_hierarchy_is_applied_with_the_appliers_visits(oracle):
    """caching 10: the hierarchy stored by a solve with one visit, applied by the same field with two -- on newer
    coefficients, so the fine level's products are the current matrix's and everything below is the stored one's."""
    case = synthetic.poisson_case(10)
    r = base.rhs(case.n_cells)
    reg = capi.Registry()
    refs, zs, aggs = [], [], []
    for step, gamma in ((0, 1), (1, 2)):
        cs = base.scaled(case, 1.0 + 0.5 * step, slice(0, case.n_cells, 3))
        refs.append(VisitRef(oracle, *oracle_csr(oracle, cs), **dict(DEFAULTS, aggregation="hashed", aggregatePasses=2)))
        s = device(reg, "v_cache", cs, "hashed", 2, gamma, caching=10)
        zs.append(s.apply_preconditioner(r))
        aggs.append(s.mg_level(0)[3].copy())
        assert s.get_property("coarseVisits") == gamma
    reg.close()
    assert refs[0].levels >= 3 and not np.array_equal(refs[1].agg[0], refs[0].agg[0])
    for step, gamma in ((0, 1), (1, 2)):
        np.testing.assert_array_equal(aggs[step], refs[0].agg[0], err_msg=f"step {step}")
        np.testing.assert_array_equal(zs[step], refs[0].with_gamma(gamma).apply(r, fine=refs[step].A[0]),
                                      err_msg=f"step {step}")
    assert not np.array_equal(zs[1], refs[0].with_gamma(1).apply(r, fine=refs[1].A[0]))


def test_time_steps_leave_no_memory_behind():
    """20 time steps with hashed / 3 that alternate between two coefficient sets and between one and two visits: the
    ledger stands still after the first four, and nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    sets = [case, base.scaled(case, 1.5, slice(0, case.n_cells, 3))]
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(20):
        s = reg.solver("v_steps", base.cfg()).set_multigrid(aggregation="hashed", aggregatePasses=3,
                                                            coarseVisits=1 + step % 2)
        s.set_matrix(sets[step % 2]).solve(b, np.zeros_like(b))
        assert s.get_property("coarseVisits") == 1 + step % 2
        if step in (3, 19):
            marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[19][k] == marks[3][k], (k, marks)
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
