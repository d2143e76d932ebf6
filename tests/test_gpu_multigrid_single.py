"""Preconditioner Multigrid with `cyclePrecision single` ("the cycle in single precision") against the
NumPy walk of its contract (tests/mg_single_walk.py, built on the double cycle's references): z = M^-1 r of
ogl_solver_apply_preconditioner bit for bit -- in the tail and launch by launch, on every in-loop layout, through a
renumbering and on a stored hierarchy --, whole solves against the oracle's loops with the walk called back as their
preconditioner, the overflow failures, and the keyword's behaviour around it (default, switching back, memory)."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import mg_single_walk as sw  # noqa: E402
import mixed_walk as mw  # noqa: E402
import precond_cases as pc  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
import test_gpu_precond_solves as solves  # noqa: E402
from test_gpu_multigrid_visits import VisitRef, visits_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = base.DEFAULTS
PLAIN = ("pgm", 1, 1)  # (aggregation, aggregatePasses, coarseVisits): the defaults

CASES = {
    "block_10_9_7": lambda: synthetic.poisson_block(10, 9, 7),            # 630 rows: two chunks, every coarse level in the tail
    "poisson14": lambda: synthetic.poisson_case(14),                      # 2,744 rows: levels 1 and 2 are launched
    "poisson12_asym": lambda: synthetic.poisson_case(12, symmetric=False),
    "voronoi": lambda: synthetic.voronoi_case(3000),
    "periodic_x": lambda: synthetic.poisson_block(10, 8, 6, periodic_x=True),  # repeated columns
    "poisson10": lambda: synthetic.poisson_case(10),
}
_cases, _refs = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def ref_of(oracle, name, variant=PLAIN, case=None):
    """The double reference of a named case (or of `case` under that name) and its single walk, each built once."""
    key = (name, variant)
    if key not in _refs:
        aggregation, passes, gamma = variant
        ref = VisitRef(oracle, *oracle_csr(oracle, case if case is not None else case_of(name)),
                       **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes)).with_gamma(gamma)
        _refs[key] = (ref, sw.SingleWalk(ref))
    return _refs[key]


def mg_of(variant=PLAIN, precision="single"):
    mg = dict(aggregation=variant[0], aggregatePasses=variant[1], coarseVisits=variant[2])
    if precision is not None:
        mg["cyclePrecision"] = precision
    return mg


def device(reg, name, case, variant=PLAIN, precision="single", props=(), **kw):
    return base.device(reg, name, case, mg=mg_of(variant, precision), props=props, **kw)


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _refs.clear()
    _cases.clear()


def assert_single(s, walk, r, fine=None, msg=""):
    assert s.get_property("mgCyclePrecisionInUse") == 1.0
    want = walk.apply(r, fine=fine)
    assert walk.smallest_fp32 >= mw.TINY32, walk.smallest_fp32  # (subnormal intermediates are not pinned: none here)
    np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=msg)
    return want


# ---- 1. the apply ----
@pytest.mark.parametrize("half", [1, 0], ids=["half", "full"])
def test_every_coarse_level_in_the_tail(oracle, reg, half):
    case = case_of("block_10_9_7")
    ref, walk = ref_of(oracle, "block_10_9_7")
    assert case.n_cells == 630 and ref.levels >= 3 and ref.A[1].n <= 512
    s = device(reg, f"s_tail_{half}", case, symmetric_half=half)
    assert s.get_property("symmetricHalf") == half
    r = base.rhs(case.n_cells)
    z = assert_single(s, walk, r)
    assert s.get_property("mgTailLevels") == ref.levels - 1
    # (jacobi0, two products, the restriction, the tail, the prolongation, two products)
    assert s.get_property("mgLaunchesPerApply") == 8
    assert not np.array_equal(z, ref.apply(r))  # (and it is not the double cycle)


@pytest.mark.parametrize("variant", [PLAIN, ("hashed", 2, 2)], ids=["defaults", "hashed-2-2"])
def test_launched_levels_and_the_tail(oracle, reg, variant):
    case = case_of("poisson14")
    ref, walk = ref_of(oracle, "poisson14", variant)
    rows = [A.n for A in ref.A]
    if variant == PLAIN:
        assert rows[0] == 2744 and rows[2] > 512 >= rows[3], rows
    else:
        assert ref.levels >= 4 and rows[1] > 512, rows  # (a launched level and revisited levels in the tail)
    s = device(reg, "s_p14", case, variant)
    assert_single(s, walk, base.rhs(case.n_cells))
    assert s.get_property("mgTailLevels") == sum(1 for n in rows if n <= 512)
    assert s.get_property("coarseVisits") == variant[2] and walk.visits == visits_of(ref.levels, variant[2])


def test_asymmetric_under_bicgstab(oracle, reg):
    case = case_of("poisson12_asym")
    ref, walk = ref_of(oracle, "poisson12_asym")
    s = device(reg, "s_asym", case, solver=capi.SOLVER_BICGSTAB)
    assert_single(s, walk, base.rhs(case.n_cells))


@pytest.mark.parametrize("name", ["voronoi", "periodic_x"])
def test_irregular_patterns(oracle, reg, name):
    case = case_of(name)
    ref, walk = ref_of(oracle, name)
    assert ref.levels >= 3
    assert_single(device(reg, "s_" + name, case), walk, base.rhs(case.n_cells))


@pytest.mark.parametrize("layout", sorted(base.LAYOUTS))
def test_every_in_loop_layout(oracle, reg, layout):
    case = case_of("poisson14")
    ref, walk = ref_of(oracle, "poisson14")
    kw, (lay, half) = base.LAYOUTS[layout]
    s = device(reg, "s_lay_" + layout, case, props=(("streamAboveBytes", 0.0),), **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    assert_single(s, walk, base.rhs(case.n_cells))


def test_renumbered_equals_caller_numbering(oracle, reg):
    case = synthetic.renumber_case(case_of("poisson14"), 4096)
    ref, walk = ref_of(oracle, "shuffled14", case=case)
    r = base.rhs(case.n_cells)
    z0 = assert_single(device(reg, "s_rn_off", case, renumber=capi.RENUMBER_OFF), walk, r)
    s1 = device(reg, "s_rn_on", case, renumber=capi.RENUMBER_ON)
    assert s1.get_property("renumbered") == 1.0
    np.testing.assert_array_equal(s1.apply_preconditioner(r), z0)
    assert s1.get_property("mgCyclePrecisionInUse") == 1.0
    base.assert_hierarchy(s1, ref)  # (the hierarchy handed out is the fp64 one, as ever)


@pytest.mark.parametrize("tail", [0.0, 1e9], ids=["no-tail", "all-in-the-tail"])
def test_wherever_the_tail_starts(oracle, reg, tail):
    """mgTailRows 0: launch by launch, the coarsest CG included.  Beyond the fine level: level 0 is launched all the same
    (it arrives and leaves in fp64), everything below it is one launch."""
    case = case_of("poisson14")
    ref, walk = ref_of(oracle, "poisson14")
    s = device(reg, "s_tailrows", case, props=(("mgTailRows", tail),))
    assert_single(s, walk, base.rhs(case.n_cells))
    assert s.get_property("mgTailLevels") == (0 if tail == 0.0 else ref.levels - 1)
    if tail:
        assert s.get_property("mgLaunchesPerApply") == 8


@pytest.mark.parametrize("what", ["maxLevels0", "coarseSolverIters0"])
def test_edges(oracle, reg, what):
    """A hierarchy of one level (the CG runs on fl32(r) and z is its x, widened) and a coarsest level without a solve."""
    case = case_of("block_10_9_7")
    mg = dict(maxLevels=0) if what == "maxLevels0" else dict(coarseSolverIters=0)
    ref = VisitRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation="pgm", aggregatePasses=1, **mg))
    assert ref.levels == 1 or what != "maxLevels0"
    s = base.device(reg, "s_" + what, case, mg=dict(mg, cyclePrecision="single"))
    assert_single(s, sw.SingleWalk(ref), base.rhs(case.n_cells))


def test_stored_hierarchy_with_the_current_fine_matrix(oracle):
    """caching 2, the coefficients rescaled at the second solve: the stored hierarchy (twin included) with the current fine
    matrix's products."""
    case = case_of("poisson10")
    r = base.rhs(case.n_cells)
    reg = capi.Registry()
    refs, zs = [], []
    for step in range(2):
        cs = base.scaled(case, 1.0 + 0.5 * step, slice(0, case.n_cells, 3))
        refs.append(VisitRef(oracle, *oracle_csr(oracle, cs), **dict(DEFAULTS, aggregation="pgm", aggregatePasses=1)))
        s = device(reg, "s_cache", cs, caching=2)
        assert s.get_property("mgCyclePrecisionInUse") == 1.0
        zs.append(s.apply_preconditioner(r))
    reg.close()
    walk = sw.SingleWalk(refs[0])
    np.testing.assert_array_equal(zs[0], walk.apply(r))
    np.testing.assert_array_equal(zs[1], walk.apply(r, fine=refs[1].A[0]))
    assert not np.array_equal(zs[1], sw.SingleWalk(refs[1]).apply(r))  # (not the hierarchy of the newer coefficients)


# ---- 2. whole solves ----
# (solver kind, case, tolerance).  GKOBiCGStab at 1e-8: with the single walk as its preconditioner the oracle's BiCGStab
# follows the double solve down to 6e-9 on this system (61 half steps against 62 at 1e-8) and then stalls at 1.36e-9 -- at
# precond_cases' 1e-9 it runs into maxIter where the double cycle needs 71 half steps (DESIGN.md section 7b says so).  A
# reference that does not stop by its tolerance pins no stop, so this case asks for 1e-8.
WHOLE = {"cg": ("poisson14", capi.SOLVER_CG, pc.TOL), "gmres": ("poisson14", capi.SOLVER_GMRES, pc.TOL),
         "bicgstab": ("poisson12_asym", capi.SOLVER_BICGSTAB, 1e-8)}


@pytest.mark.parametrize("solver", sorted(WHOLE))
def test_whole_solves_are_the_oracles(oracle, reg, solver):
    name, kind, tolerance = WHOLE[solver]
    case = case_of(name)
    _, walk = ref_of(oracle, name)
    b, xs = synthetic.rhs_for_x_star(case)
    rp, cols, vals = oracle_csr(oracle, case)
    ref = pc.oracle_solve(oracle.DistMatrix(rp, cols, vals), b, pc.callback(walk.apply), solver, tolerance=tolerance)
    assert walk.smallest_fp32 >= mw.TINY32
    assert ref.final_residual <= tolerance and 3 <= ref.n_iterations < pc.MAX_ITER, (ref.n_iterations, ref.final_residual)
    cfg = capi.default_config(solver=kind, preconditioner=capi.PRECOND_MULTIGRID, tolerance=tolerance, rel_tol=0.0,
                              max_iter=pc.MAX_ITER, export_res=1, adapt_min_iter=0, renumber=capi.RENUMBER_OFF,
                              krylov_dim=pc.KRYLOV_DIM, update_init_guess=1)
    s = reg.solver("s_whole_" + solver, cfg).set_multigrid(**dict(DEFAULTS, cyclePrecision="single")).set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("mgCyclePrecisionInUse") == 1.0
    true = mw.true_residual(oracle, rp, cols, vals, b, x, perf.norm_factor)
    print(solver, "iterations", perf.n_iterations, "true residual", true, "final", perf.final_residual)
    solves.assert_is_the_oracles((s, x, perf, s.history()), ref, solver)
    assert mw.meets_criterion(true, perf.initial_residual, tolerance, 0.0)
    assert np.abs(x - xs).max() <= 1e-5


# ---- 3. failures ----
def solve_fails(s, case, words):
    b = np.ones(case.n_cells)
    for _ in range(2):  # (the second solve must convert -- and report -- again)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, np.zeros_like(b))
        assert e.value.status == capi.ERR_INVALID, e.value
        for w in words:
            assert w in str(e.value), e.value


@pytest.mark.parametrize("half", [1, 0], ids=["half", "csr"])
def test_a_fine_coefficient_beyond_binary32_fails_the_solve(reg, half):
    case = copy.deepcopy(case_of("block_10_9_7"))
    case.diag[577] = 1e39
    s = reg.solver(f"s_over0_{half}", base.cfg(symmetric_half=half, compress_indices=half))
    s.set_multigrid(**dict(DEFAULTS, cyclePrecision="single")).set_matrix(case)
    solve_fails(s, case, ("Multigrid", "cyclePrecision", "level 0", "row 577"))
    # (the same matrix in double precision is a solvable system still)
    s.set_multigrid(cyclePrecision="double")
    s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert s.get_property("mgCyclePrecisionInUse") == 0.0


def test_a_galerkin_sum_beyond_binary32_fails_the_solve(oracle, reg):
    """Rows 100 and 101 (neighbours in x) with diagonals of 3e38 and -1e38 between them: each is the other's strongest
    neighbour, and their aggregate's diagonal, 4e38, is finite in double precision only.  Level 0 itself converts."""
    case = copy.deepcopy(case_of("block_10_9_7"))
    f = np.flatnonzero((case.lower_addr == 100) & (case.upper_addr == 101))
    assert f.size == 1
    case.diag[[100, 101]] = 3e38
    case.upper[f[0]] = -1e38
    ref = VisitRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation="pgm", aggregatePasses=1))
    assert ref.agg[0][100] == ref.agg[0][101]
    assert np.all(np.isfinite(ref.A[0].vals.astype(np.float32)))
    with np.errstate(over="ignore"):
        assert not np.all(np.isfinite(ref.A[1].vals.astype(np.float32)))
    s = reg.solver("s_over1", base.cfg()).set_multigrid(**dict(DEFAULTS, cyclePrecision="single")).set_matrix(case)
    solve_fails(s, case, ("Multigrid", "level 1", f"row {ref.agg[0][100]} "))


@pytest.mark.parametrize("value", [2, 0.5])
def test_refusals(reg, value):
    case = synthetic.poisson_case(6)
    s = reg.solver(f"s_refuse_{value}", base.cfg()).set_multigrid(cyclePrecision=value).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == capi.ERR_INVALID and "cyclePrecision" in str(e.value), e.value


def test_an_unknown_word_is_refused_at_the_boundary(reg):
    with pytest.raises(KeyError):
        reg.solver("s_word", base.cfg()).set_multigrid(cyclePrecision="half")


# ---- 4. around the keyword ----
def test_unset_and_zero_are_the_double_cycle(oracle, reg):
    case = case_of("poisson14")
    ref, _ = ref_of(oracle, "poisson14")
    r = base.rhs(case.n_cells)
    want = ref.apply(r)
    for precision in (None, "double", 0):
        s = device(reg, f"s_default_{precision}", case, precision=precision)
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"cyclePrecision {precision}")
        assert s.get_property("mgCyclePrecisionInUse") == 0.0


def test_switching_back_gives_the_double_bits_again(oracle, reg):
    case = case_of("poisson14")
    ref, walk = ref_of(oracle, "poisson14")
    r = base.rhs(case.n_cells)
    for precision, want in (("single", walk.apply(r)), ("double", ref.apply(r)), ("single", walk.apply(r))):
        s = device(reg, "s_switch", case, precision=precision)
        np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=precision)
        assert s.get_property("mgCyclePrecisionInUse") == (1.0 if precision == "single" else 0.0)


def test_alternating_precisions_leave_the_ledger_still_from_the_third_step():
    """A time-step loop on one field that alternates double and single: the twin, the fp32 copy of the fine level and the
    fp32 vectors are there after the first single step (the second step), on the registry's hierarchy or this field's own;
    the drift of the ledger is exactly 0 from the third step, and nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(8):
        s = reg.solver("s_steps", base.cfg()).set_multigrid(cyclePrecision=step % 2)
        s.set_matrix(case).solve(b, np.zeros_like(b))
        assert s.get_property("mgCyclePrecisionInUse") == step % 2
        marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for step in range(3, 8):
        for k in soak_worker.LEDGER_EXACT:
            assert marks[step][k] == marks[2][k], (step, k, marks[step][k], marks[2][k])
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
