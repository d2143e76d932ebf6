"""Preconditioner Multigrid with `smootherSweeps nu` and `correctionScale alpha` ("sweeps and
correction scale"): nu sweeps before and after the coarse correction on every level, and the correction added as
t = x + alpha x_c[agg].  The references are the walks of tests/mg_smoother_walk.py -- VisitRef and SingleWalk with only
`cycle` overridden to that contract.  z = M^-1 r bit for bit wherever the single-workgroup tail starts, on every in-loop
layout, renumbered, in single precision and on a stored hierarchy; whole solves against the oracle's loops with the walk
called back as their preconditioner; the defaults, the refusals and the allocation ledger."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import mg_smoother_walk as smw  # noqa: E402
import mixed_walk as mw  # noqa: E402
import precond_cases as pc  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
import test_gpu_precond_solves as solves  # noqa: E402
from test_gpu_multigrid_aggregation import PassRef  # noqa: E402
from test_gpu_multigrid_visits import visits_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = base.DEFAULTS
VARIANTS = [(1, 1.0), (1, 1.25), (3, 1.5), (4, 1.0), (2, 1.5)]  # (smootherSweeps, correctionScale); 3: the odd ping-pong parity
HIERARCHIES = [("hashed", 2), ("pgm", 1)]
CASES = dict(base.CASES)
CASES.update({
    "poisson14": lambda: synthetic.poisson_case(14),                      # 2,744 rows: launched coarse levels under pgm / 1
    "block_10_9_7": lambda: synthetic.poisson_block(10, 9, 7),            # 630 rows: every coarse level in the tail
    "poisson12_asym": lambda: synthetic.poisson_case(12, symmetric=False),
    "shuffled14": lambda: synthetic.renumber_case(synthetic.poisson_case(14), 4096),
})
_cases, _refs = {}, {}


# ---------------------------------------------------------------------------------------------------------------------
# reference and device
# ---------------------------------------------------------------------------------------------------------------------
def case_of(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def ref_of(oracle, name, aggregation, passes, nu, alpha, gamma=1, iters=4):
    """(case, walk) of a named case; every hierarchy is built once and shared by its walks (the hierarchy does not depend
    on coarseSolverIters)."""
    key = (name, aggregation, passes)
    if key not in _refs:
        _refs[key] = smw.SmoothRef(oracle, *oracle_csr(oracle, case_of(name)),
                                   **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    walk = _refs[key].with_smoother(nu, alpha, gamma)
    walk.iters = iters
    return case_of(name), walk


def mg_of(aggregation, passes, nu, alpha, gamma=None, **mg):
    mg = dict(mg, aggregation=aggregation, aggregatePasses=passes)
    for key, value in (("smootherSweeps", nu), ("correctionScale", alpha), ("coarseVisits", gamma)):
        if value is not None:
            mg[key] = value
    return mg


def device(reg, name, case, aggregation, passes, nu, alpha, gamma=None, mg=None, props=(), **kw):
    return base.device(reg, name, case, mg=mg_of(aggregation, passes, nu, alpha, gamma, **(mg or {})), props=props, **kw)


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _refs.clear()
    _cases.clear()


def assert_keywords(s, walk):
    assert s.get_property("smootherSweeps") == walk.nu and s.get_property("correctionScale") == walk.alpha
    assert s.get_property("coarseVisits") == walk.gamma
    assert walk.visits == visits_of(walk.levels, walk.gamma)
    for l, v in enumerate(walk.visits):
        assert s.get_property(f"mgVisits{l}") == v, (l, walk.visits)


def assert_single(s, walk, r, fine=None, msg=""):
    assert s.get_property("mgCyclePrecisionInUse") == 1.0
    want = walk.apply(r, fine=fine)
    assert walk.smallest_fp32 >= mw.TINY32, walk.smallest_fp32  # (subnormal intermediates are not pinned: none here)
    np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=msg)
    return want


# ---- 1. the apply ----
APPLY = [(name, v) for name in sorted(base.CASES) for v in ((1, 1.25), (3, 1.5))] + \
        [("poisson_sym", v) for v in VARIANTS if v not in ((1, 1.25), (3, 1.5))]


@pytest.mark.parametrize("name,variant", APPLY, ids=lambda v: str(v))
def test_apply_bit_identical(oracle, reg, name, variant):
    """z = M^-1 r on hashed / 2 and pgm / 1 for coarseSolverIters 4 and 0 (default tail), and both keywords read back."""
    nu, alpha = variant
    for aggregation, passes in HIERARCHIES:
        for iters in (4, 0):
            case, walk = ref_of(oracle, name, aggregation, passes, nu, alpha, iters=iters)
            assert walk.levels >= 3
            r = base.rhs(case.n_cells)
            s = device(reg, f"sm_{name}", case, aggregation, passes, nu, alpha, mg=dict(coarseSolverIters=iters))
            np.testing.assert_array_equal(s.apply_preconditioner(r), walk.apply(r),
                                          err_msg=f"{name} {aggregation} / {passes} iters {iters}")
            assert_keywords(s, walk)


@pytest.mark.parametrize("aggregation,passes", HIERARCHIES)
def test_two_sweeps_unscaled_launch_what_the_unset_keywords_launch(oracle, reg, aggregation, passes):
    case = case_of("poisson_sym")
    r = base.rhs(case.n_cells)
    launches, zs = {}, {}
    for tail in (0.0, 512.0):
        for nu, alpha in ((None, None), (2, 1.0), (1, 1.0), (3, 1.0)):
            # (a field of its own each: a keyword left unset must not be the one a solve before has set)
            s = device(reg, f"sm_launch_{aggregation}_{tail}_{nu}", case, aggregation, passes, nu, alpha,
                       props=(("mgTailRows", tail),))
            zs[tail, nu] = s.apply_preconditioner(r)
            launches[tail, nu] = s.get_property("mgLaunchesPerApply")
        np.testing.assert_array_equal(zs[tail, 2], zs[tail, None])
        assert launches[tail, 2] == launches[tail, None], launches
        # (a sweep less / more before and after the correction on every launched level: the count moves with it)
        assert launches[tail, 1] < launches[tail, 2] < launches[tail, 3], launches
    print("launches per apply", launches)


# ---- 2. where the tail starts ----
@pytest.mark.parametrize("gamma", [1, 2])
@pytest.mark.parametrize("variant", [(1, 1.25), (3, 1.5)], ids=str)
def test_apply_bit_identical_wherever_the_tail_starts(oracle, reg, variant, gamma):
    """mgTailRows 0 (no tail), the rows of the last level, of level 2 (with coarseVisits 2 the tail's first level is
    continued by the host: nu full pre-sweeps from a guess inside the kernel), of level 1 (the recursion inside the
    kernel) and n + 1 (one launch)."""
    nu, alpha = variant
    case, walk = ref_of(oracle, "poisson_sym", "hashed", 2, nu, alpha, gamma)
    rows = [A.n for A in walk.A]
    assert walk.levels >= 4 and len(set(rows)) == len(rows), rows
    r = base.rhs(case.n_cells)
    want = walk.apply(r)
    for tail in (0.0, float(rows[-1]), float(rows[2]), float(rows[1]), float(case.n_cells + 1)):
        s = device(reg, "sm_tail", case, "hashed", 2, nu, alpha, gamma, props=(("mgTailRows", tail),))
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"tail {tail}")
        assert s.get_property("mgTailLevels") == sum(1 for n in rows if n <= tail), tail
        assert_keywords(s, walk)
        if tail > case.n_cells:
            assert s.get_property("mgLaunchesPerApply") == 1


# ---- 3. every fine-level layout, and renumbered ----
@pytest.mark.parametrize("layout", sorted(base.LAYOUTS))
def test_apply_bit_identical_on_every_layout(oracle, reg, layout):
    case, walk = ref_of(oracle, "poisson_sym", "hashed", 2, 1, 1.25)
    r = base.rhs(case.n_cells)
    kw, (lay, half) = base.LAYOUTS[layout]
    s = device(reg, "sm_lay_" + layout, case, "hashed", 2, 1, 1.25, props=(("streamAboveBytes", 0.0),), **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    np.testing.assert_array_equal(s.apply_preconditioner(r), walk.apply(r))


@pytest.mark.parametrize("variant", [(1, 1.25), (3, 1.5)], ids=str)
def test_renumbered_equals_caller_numbering(oracle, reg, variant):
    """(3, 1.5) too: the fine level keeps a CSR matrix of its own here, and its sweeps are the launched CSR ones.)"""
    nu, alpha = variant
    case, walk = ref_of(oracle, "shuffled14", "hashed", 2, nu, alpha)
    r = base.rhs(case.n_cells)
    want = walk.apply(r)
    s0 = device(reg, "sm_rn_off", case, "hashed", 2, nu, alpha, renumber=capi.RENUMBER_OFF)
    np.testing.assert_array_equal(s0.apply_preconditioner(r), want)
    s1 = device(reg, "sm_rn_on", case, "hashed", 2, nu, alpha, renumber=capi.RENUMBER_ON)
    assert s1.get_property("renumbered") == 1.0
    assert not np.array_equal(s1.renumbering(), np.arange(case.n_cells))
    np.testing.assert_array_equal(s1.apply_preconditioner(r), want)


# ---- 4. cyclePrecision single ----
SINGLE = [("block_10_9_7", "pgm", 1, 1, "half"), ("block_10_9_7", "pgm", 1, 1, "csr_stream"),  # every coarse level in the tail
          ("poisson14", "pgm", 1, 1, "half"), ("poisson14", "pgm", 1, 1, "csr_stream"),        # launched coarse levels
          ("poisson14", "hashed", 2, 2, "half")]                                               # coarseVisits 2


@pytest.mark.parametrize("variant", [(1, 1.25), (3, 1.5)], ids=str)
@pytest.mark.parametrize("name,aggregation,passes,gamma,layout", SINGLE, ids=lambda v: str(v))
def test_single_precision_bit_identical(oracle, reg, name, aggregation, passes, gamma, layout, variant):
    nu, alpha = variant
    case, ref = ref_of(oracle, name, aggregation, passes, nu, alpha, gamma)
    walk = smw.SmoothSingle(ref)
    assert (walk.nu, walk.gamma) == (nu, gamma) and walk.alpha == np.float32(alpha)
    rows = [A.n for A in ref.A]
    if name == "block_10_9_7":
        assert rows[1] <= 512
    elif aggregation == "pgm":
        assert rows[2] > 512 >= rows[-1], rows
    else:
        assert ref.levels >= 4 and rows[1] > 512, rows
    kw, (lay, half) = base.LAYOUTS[layout]
    s = device(reg, f"sm_single_{layout}", case, aggregation, passes, nu, alpha, gamma, mg=dict(cyclePrecision="single"), **kw)
    assert s.get_property("symmetricHalf") == half
    r = base.rhs(case.n_cells)
    z = assert_single(s, walk, r)
    assert s.get_property("mgTailLevels") == sum(1 for n in rows[1:] if n <= 512)
    assert s.get_property("smootherSweeps") == nu and s.get_property("correctionScale") == alpha
    assert walk.visits == visits_of(ref.levels, gamma)
    assert not np.array_equal(z, ref.apply(r))  # (and it is not the double cycle)


def test_single_precision_launch_by_launch_and_renumbered(oracle, reg):
    """mgTailRows 0: the coarse levels' sweeps and the coarsest CG launch by launch; renumber on: the fine level's CSR twin,
    whose last post-sweep writes the doubles."""
    case, ref = ref_of(oracle, "shuffled14", "hashed", 2, 3, 1.5)
    walk = smw.SmoothSingle(ref)
    r = base.rhs(case.n_cells)
    s = device(reg, "sm_single_notail", case, "hashed", 2, 3, 1.5, mg=dict(cyclePrecision="single"),
               props=(("mgTailRows", 0.0),))
    want = assert_single(s, walk, r)
    assert s.get_property("mgTailLevels") == 0
    s = device(reg, "sm_single_rn", case, "hashed", 2, 3, 1.5, mg=dict(cyclePrecision="single"), renumber=capi.RENUMBER_ON)
    assert s.get_property("renumbered") == 1.0 and s.get_property("mgCyclePrecisionInUse") == 1.0
    np.testing.assert_array_equal(s.apply_preconditioner(r), want)


# ---- 5. whole solves ----
WHOLE = {"cg": ("poisson14", capi.SOLVER_CG), "gmres": ("poisson14", capi.SOLVER_GMRES),
         "bicgstab": ("poisson12_asym", capi.SOLVER_BICGSTAB)}


@pytest.mark.parametrize("solver", sorted(WHOLE))
def test_whole_solves_are_the_oracles(oracle, reg, solver):
    """One sweep, the correction scaled by 1.25, on hashed / 3 (the hierarchy the keywords are meant for): the oracle's loop
    with the walk called back.  On hashed / 2 the oracle's restarted GMRES(20) stagnates on this system with these values
    (7e-7 at maxIter, where two unscaled sweeps need 82 turns): a reference that does not stop by its tolerance pins no
    stop."""
    name, kind = WHOLE[solver]
    case, walk = ref_of(oracle, name, "hashed", 3, 1, 1.25)
    b, xs = synthetic.rhs_for_x_star(case)
    rp, cols, vals = oracle_csr(oracle, case)
    ref = pc.oracle_solve(oracle.DistMatrix(rp, cols, vals), b, pc.callback(walk.apply), solver)
    # (the reference pins something: it stops by the tolerance, before max_iter, at the solution)
    assert ref.final_residual <= pc.TOL and 3 <= ref.n_iterations < pc.MAX_ITER, (ref.n_iterations, ref.final_residual)
    assert np.abs(ref.x - xs).max() <= 1e-6
    cfg = capi.default_config(solver=kind, preconditioner=capi.PRECOND_MULTIGRID, tolerance=pc.TOL, rel_tol=0.0,
                              max_iter=pc.MAX_ITER, export_res=1, adapt_min_iter=0, renumber=capi.RENUMBER_OFF,
                              krylov_dim=pc.KRYLOV_DIM, update_init_guess=1)
    s = reg.solver("sm_whole_" + solver, cfg).set_multigrid(**mg_of("hashed", 3, 1, 1.25, **DEFAULTS)).set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    print(solver, "iterations", perf.n_iterations, "final", perf.final_residual)
    assert s.get_property("smootherSweeps") == 1 and s.get_property("correctionScale") == 1.25
    solves.assert_is_the_oracles((s, x, perf, s.history()), ref, solver)


# ---- 6. the defaults, switching back, a shared hierarchy ----
def test_unset_and_the_defaults_set_are_todays_cycle(oracle, reg):
    case, walk = ref_of(oracle, "poisson_sym", "hashed", 2, 2, 1.0, gamma=2)
    r = base.rhs(case.n_cells)
    want = walk.as_visit_ref().apply(r)
    for nu, alpha in ((None, None), (2, 1.0), (2, None), (None, 1.0)):
        s = device(reg, f"sm_default_{nu}_{alpha}", case, "hashed", 2, nu, alpha, 2)
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{nu} {alpha}")
        assert s.get_property("smootherSweeps") == 2 and s.get_property("correctionScale") == 1.0
    # (one visit, defaults: PassRef's own V-cycle)
    plain = copy.copy(walk)
    plain.__class__ = PassRef
    s = device(reg, "sm_default_plain", case, "hashed", 2, None, None)
    np.testing.assert_array_equal(s.apply_preconditioner(r), plain.apply(r))


def test_switching_back_gives_todays_bits_again(oracle, reg):
    case, walk = ref_of(oracle, "poisson_sym", "hashed", 2, 1, 1.25)
    r = base.rhs(case.n_cells)
    today = walk.as_visit_ref().apply(r)
    other = walk.apply(r)
    assert not np.array_equal(today, other)
    for (nu, alpha), want in (((2, 1.0), today), ((1, 1.25), other), ((2, 1.0), today), ((1, 1.25), other)):
        s = device(reg, "sm_switch", case, "hashed", 2, nu, alpha)
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{nu} {alpha}")
        assert s.get_property("smootherSweeps") == nu and s.get_property("correctionScale") == alpha


def test_two_solvers_apply_one_stored_hierarchy_each_with_its_own_values(oracle):
    """caching 5: field A generates and stores the hierarchy.  Field B, on newer coefficients, generates its own for its
    first solve (its counter starts at 0, as every field's) and applies the stored one from its second -- the fine level's
    products are its own matrix's -- with other sweeps and another scale; then A again with its own values."""
    case = synthetic.poisson_case(10)
    r = base.rhs(case.n_cells)
    newer = base.scaled(case, 1.5, slice(0, case.n_cells, 3))
    refs = [smw.SmoothRef(oracle, *oracle_csr(oracle, c), **dict(DEFAULTS, aggregation="hashed", aggregatePasses=2))
            for c in (case, newer)]
    assert refs[0].levels >= 3 and not np.array_equal(refs[1].agg[0], refs[0].agg[0])
    reg = capi.Registry()
    zs = []
    # (field, its matrix, its keywords, the hierarchy it applies)
    steps = (("A", case, (1, 1.25), 0), ("B", newer, (3, 1.5), 1), ("B", newer, (3, 1.5), 0), ("A", case, (1, 1.25), 0))
    for field, c, (nu, alpha), which in steps:
        s = device(reg, "sm_shared_" + field, c, "hashed", 2, nu, alpha, caching=5)
        zs.append(s.apply_preconditioner(r))
        assert s.get_property("smootherSweeps") == nu and s.get_property("correctionScale") == alpha
        np.testing.assert_array_equal(s.mg_level(0)[3], refs[which].agg[0], err_msg=field)
    reg.close()
    np.testing.assert_array_equal(zs[0], refs[0].with_smoother(1, 1.25).apply(r))
    np.testing.assert_array_equal(zs[1], refs[1].with_smoother(3, 1.5).apply(r))
    np.testing.assert_array_equal(zs[2], refs[0].with_smoother(3, 1.5).apply(r, fine=refs[1].A[0]))
    np.testing.assert_array_equal(zs[3], zs[0])
    assert not np.array_equal(zs[2], zs[1])  # (not the hierarchy of the newer coefficients)


# ---- 7. refusals ----
@pytest.mark.parametrize("key,value", [("smootherSweeps", 0), ("smootherSweeps", 5), ("smootherSweeps", 1.5),
                                       ("correctionScale", 0), ("correctionScale", 2), ("correctionScale", -1),
                                       ("correctionScale", float("nan")), ("correctionScale", float("inf"))],
                         ids=lambda v: str(v))
def test_refusals(reg, key, value):
    case = synthetic.poisson_case(6)
    s = reg.solver(f"sm_refuse_{key}_{value}", base.cfg()).set_multigrid(**{key: value}).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == capi.ERR_INVALID and key in str(e.value), e.value
    assert f"{float(value):g}" in str(e.value), e.value


def test_an_unknown_keyword_is_refused_at_the_boundary(reg):
    with pytest.raises(KeyError):
        reg.solver("sm_word", base.cfg()).set_multigrid(smootherSweep=1)
    with pytest.raises(KeyError):
        reg.solver("sm_word", base.cfg()).set_multigrid(correctionScales=1.25)


# ---- 8. memory ----
def test_alternating_sweeps_and_scales_leave_the_ledger_still_from_the_third_step():
    """A time-step loop on one field that alternates (2, 1.0) and (1, 1.25): neither keyword allocates anything, so the
    drift of the ledger is exactly 0 from the third step, and nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(8):
        nu, alpha = ((2, 1.0), (1, 1.25))[step % 2]
        s = reg.solver("sm_steps", base.cfg()).set_multigrid(aggregation="hashed", aggregatePasses=3, smootherSweeps=nu,
                                                             correctionScale=alpha)
        s.set_matrix(case).solve(b, np.zeros_like(b))
        assert s.get_property("smootherSweeps") == nu and s.get_property("correctionScale") == alpha
        marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for step in range(3, 8):
        for k in soak_worker.LEDGER_EXACT:
            assert marks[step][k] == marks[2][k], (step, k, marks[step][k], marks[2][k])
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
