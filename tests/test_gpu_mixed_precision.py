"""GPU tests of the mixed-precision mode of GKOCG (property mixedPrecision): fp32 Krylov turns on an
fp32 copy of the matrix as the inner solver of an fp64 iterative refinement.  The contract is the NumPy walk of
tests/mixed_walk.py, and everything here is compared with it bit for bit: the inner SpMV on both storages, whole solves
(x, counts, stop reason, exported history), the refusals, and a time-step loop that must not allocate after its first
steps.  The conditions these inputs rely on (outer steps, no subnormal fp32 intermediate) are tests/test_mixed_walk.py."""
import functools

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_matrix, oracle_matrix_renumbered, to_new
import mixed_walk as mw

pytestmark = pytest.mark.gpu

HALF, CSR = 2.0, 0.0  # property mixedInnerLayout


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def cfg(**kw):
    base = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ, max_block_size=1, tolerance=1e-10, rel_tol=0.0,
                max_iter=1000, export_res=1)
    base.update(kw)
    return capi.default_config(**base)


def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


# ---- 1. the inner SpMV ----
SPMV_CASES = {
    "10x9x7": (lambda: synthetic.poisson_block(10, 9, 7), HALF),
    "6x6x6": (lambda: synthetic.poisson_block(6, 6, 6), HALF),
    "11x10x10": (lambda: synthetic.poisson_block(11, 10, 10), HALF),   # 1100 rows: three chunks
    # the float instantiations of the shared half-storage walk with two and three planes, and a long line
    "1031x1x1": (lambda: synthetic.poisson_block(1031, 1, 1), HALF),   # two planes, pair loads: three chunks, the last partial
    "64x9x1": (lambda: synthetic.poisson_block(64, 9, 1), HALF),       # three planes, pair loads: 576 rows, two chunks
    "33x31x1": (lambda: synthetic.poisson_block(33, 31, 1), HALF),     # three planes, odd line length (plain loads): 1023 rows
    "127x1x1": (lambda: synthetic.poisson_block(127, 1, 1), HALF),     # two planes: fewer rows than one chunk
    "258x2x2": (lambda: synthetic.poisson_block(258, 2, 2), HALF),     # four planes: a line longer than a wavefront's 128 rows
    "voronoi600": (lambda: synthetic.voronoi_case(600), CSR),
    "asymmetric": (lambda: synthetic.poisson_block(10, 9, 7, symmetric=False, off_upper=-0.9, off_lower=-1.1), CSR),
}


def randomise(case, seed):
    """Coefficients that are not representable in binary32, different on every face."""
    rng = np.random.default_rng(seed)
    case.upper[:] = rng.uniform(-1.0, -0.25, case.upper.size)
    if case.lower is not None:
        case.lower[:] = rng.uniform(-1.0, -0.25, case.lower.size)
    case.diag[:] = rng.uniform(7.0, 9.0, case.n_cells)
    return case


@pytest.mark.parametrize("name", sorted(SPMV_CASES))
def test_spmv_f32_is_the_walks_product(reg, oracle, name):
    make, layout = SPMV_CASES[name]
    case = randomise(make(), 11)
    rp, cols, vals = oracle_csr(oracle, case)
    x = np.random.default_rng(5).uniform(-1, 1, case.n_cells).astype(np.float32)
    s = reg.solver("mx_spmv_" + name, cfg()).set_matrix(case)
    y = s.spmv_f32(x)
    assert s.get_property("mixedInnerLayout") == layout
    np.testing.assert_array_equal(y, mw.spmv32(rp, cols, vals.astype(np.float32), x))


def test_spmv_f32_on_a_renumbered_device_copy(reg, oracle):
    case = randomise(synthetic.renumber_case(synthetic.poisson_case(12), 256), 12)
    s = reg.solver("mx_spmv_renumbered", cfg(renumber=capi.RENUMBER_ON)).set_matrix(case)
    new_id = s.renumbering()
    assert new_id is not None
    _, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    x = np.random.default_rng(6).uniform(-1, 1, case.n_cells).astype(np.float32)
    y = s.spmv_f32(x)
    assert s.get_property("mixedInnerLayout") == CSR
    np.testing.assert_array_equal(y, mw.spmv32(rp, cols, vals.astype(np.float32), to_new(x, new_id))[new_id])


# ---- 2. whole solves against the walk, 3. the answer is a double-precision answer ----
def box(shape):
    def make():
        case = synthetic.poisson_block(*shape)
        return case, synthetic.rhs_for_x_star(case)[0], None
    return make


def zero_rhs():
    case = synthetic.poisson_block(10, 9, 7)
    return case, np.zeros(case.n_cells), None


def start_at_the_solution():
    case = synthetic.poisson_block(10, 9, 7)
    b, xs = synthetic.rhs_for_x_star(case)
    return case, b, xs


def voronoi():
    case = synthetic.voronoi_case(600)
    rng = np.random.default_rng(8)
    return case, synthetic.apply_case(case, rng.uniform(-1, 1, case.n_cells)), None


TIGHT, LOOSE = dict(tolerance=1e-10, rel_tol=0.0), dict(tolerance=1e-10, rel_tol=0.01)
NONE, BJ1 = capi.PRECOND_NONE, capi.PRECOND_BJ
SOLVES = {}
for _shape in ((10, 9, 7), (6, 6, 6)):
    for _pname, _p in (("none", NONE), ("BJ1", BJ1)):
        for _cname, _c in (("tight", TIGHT), ("loose", LOOSE)):
            SOLVES["%dx%dx%d-%s-%s" % (*_shape, _pname, _cname)] = (box(_shape), _p, dict(_c), {})
SOLVES["innerMaxIter5"] = (box((10, 9, 7)), BJ1, dict(TIGHT), dict(inner_max_iter=5))
SOLVES["maxIter-in-second-inner-solve"] = (box((10, 9, 7)), BJ1, dict(TIGHT, max_iter="first+3"), {})
SOLVES["minIter-above-first-step"] = (box((10, 9, 7)), BJ1, dict(LOOSE, min_iter="first+1"), {})
SOLVES["zero-rhs"] = (zero_rhs, BJ1, dict(TIGHT), {})
SOLVES["start-at-solution"] = (start_at_the_solution, BJ1, dict(TIGHT), {})
SOLVES["voronoi600"] = (voronoi, BJ1, dict(TIGHT), {})


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, b, x0, criterion keywords, inner keywords, the walk): computed once per case and left unchanged."""
    from oracle import oracle
    oracle.build()
    make, precond, crit, inner = SOLVES[name]
    case, b, x0 = make()
    x0 = np.zeros_like(b) if x0 is None else x0
    rp, cols, vals = oracle_csr(oracle, case)
    inv_d = oracle.jacobi_generate_scalar(rp, cols, vals) if precond == BJ1 else None

    def run(**kw):
        with blocked(oracle, chunk_rows()):
            return mw.mixed_walk(oracle, rp, cols, vals, b, x0, inv_d, **kw, **inner)
    for key in ("max_iter", "min_iter"):  # "first+k": relative to the turns of the first outer step of the same solve
        if isinstance(crit.get(key), str):
            plain = {k: v for k, v in crit.items() if k != key}
            crit[key] = run(**plain).step_turns[0] + int(crit[key].split("+")[1])
    return case, b, x0, crit, inner, run(**crit), (rp, cols, vals)


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_solve_is_the_walk(reg, oracle, name):
    case, b, x0, crit, inner, w, (rp, cols, vals) = reference(name)
    s = reg.solver("mx_solve_" + name, cfg(preconditioner=SOLVES[name][1], **crit)).set_matrix(case)
    s.set_mixed_precision(True, inner_max_iter=inner.get("inner_max_iter"))
    x, perf = s.solve(b, x0)
    got = dict(n_iterations=perf.n_iterations, n_evals=perf.n_norm_evals, outer=s.get_property("mixedOuterSteps"),
               turns=s.get_property("mixedInnerTurns"), reason=s.get_property("mixedStopReason"))
    print(name, got, "walk:", w.n_iterations, w.n_evals, w.outer_steps, w.inner_turns, w.stop_reason, w.step_turns)
    assert s.get_property("mixedPrecisionInUse") == 1.0
    assert got == dict(n_iterations=w.n_iterations, n_evals=w.n_evals, outer=w.outer_steps, turns=w.inner_turns,
                       reason=w.stop_reason)
    np.testing.assert_array_equal(s.history(), w.history)
    np.testing.assert_array_equal(x, w.x)
    assert perf.initial_residual == w.initial_residual and perf.final_residual == w.final_residual
    if w.stop_reason == mw.STOP_CRITERION:
        true = mw.true_residual(oracle, rp, cols, vals, b, x, perf.norm_factor)
        print(name, "true residual", true, "criterion", crit)
        assert mw.meets_criterion(true, perf.initial_residual, crit["tolerance"], crit["rel_tol"])


def test_the_cases_cover_what_they_are_named_for():
    assert reference("10x9x7-BJ1-tight")[5].outer_steps >= 2 and reference("6x6x6-none-tight")[5].outer_steps >= 2
    assert reference("10x9x7-none-loose")[5].outer_steps == 1
    assert all(t == 5 for t in reference("innerMaxIter5")[5].step_turns)
    w = reference("maxIter-in-second-inner-solve")[5]
    assert w.outer_steps == 2 and w.stop_reason == mw.STOP_MAX_ITER and w.step_turns[1] == 3
    w = reference("minIter-above-first-step")[5]
    assert w.outer_steps == 2 and w.n_evals == 2
    assert reference("zero-rhs")[5].inner_turns == 0


# ---- 4. refusals, and off by default ----
@pytest.mark.parametrize("kw, names", [
    (dict(solver=capi.SOLVER_BICGSTAB), ["GKOBiCGStab"]),
    (dict(solver=capi.SOLVER_GMRES), ["GKOGMRES"]),
    (dict(max_block_size=4), ["BJ", "maxBlockSize 4"]),
    (dict(preconditioner=capi.PRECOND_ISAI), ["ISAI"]),
], ids=["BiCGStab", "GMRES", "BJ4", "ISAI"])
def test_refused_where_it_does_not_apply(reg, kw, names):
    case = synthetic.poisson_block(6, 6, 6)
    b = synthetic.rhs_for_x_star(case)[0]
    s = reg.solver("mx_refused_" + "_".join(names).replace(" ", ""), cfg(**kw)).set_matrix(case)
    s.set_mixed_precision(True)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, np.zeros_like(b))
    assert e.value.status == capi.ERR_UNSUPPORTED
    for n in names + ["1 rank"]:
        assert n in str(e.value)
    s.set_mixed_precision(False)  # ... and the same handle solves in double precision
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("mixedPrecisionInUse") == 0.0 and perf.final_residual < 1e-10


@pytest.mark.parametrize("half", [1, 0], ids=["half", "csr"])
def test_a_coefficient_beyond_binary32_fails_the_solve(reg, half):
    case = synthetic.poisson_block(10, 9, 7)
    case.diag[577] = 1e39
    b = synthetic.rhs_for_x_star(case)[0]
    s = reg.solver("mx_overflow%d" % half, cfg(symmetric_half=half, compress_indices=half)).set_matrix(case)
    s.set_mixed_precision(True)
    for _ in range(2):  # (the second solve finds the same copy and must report again)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, np.zeros_like(b))
        assert e.value.status == capi.ERR_INVALID and "row 577" in str(e.value)
    with pytest.raises(capi.OglError) as e:
        s.spmv_f32(np.ones(case.n_cells, np.float32))
    assert e.value.status == capi.ERR_INVALID and "row 577" in str(e.value)


@pytest.mark.parametrize("key, value", [("innerRelTol", 0.0), ("innerRelTol", 1.0), ("innerRelTol", -0.5),
                                        ("innerRelTol", float("nan")), ("innerMaxIter", 0.0), ("innerMaxIter", -3.0)])
def test_bad_inner_keywords(reg, key, value):
    case = synthetic.poisson_block(6, 6, 6)
    b = synthetic.rhs_for_x_star(case)[0]
    s = reg.solver("mx_bad_keyword", cfg()).set_matrix(case)
    s.set_mixed_precision(True, inner_rel_tol=1e-4, inner_max_iter=1000)
    s.set_property(key, value)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, np.zeros_like(b))
    assert e.value.status == capi.ERR_INVALID and key in str(e.value)


@pytest.mark.parametrize("setting", [None, 0.0], ids=["unset", "0"])
def test_off_by_default(reg, oracle, setting):
    case = synthetic.poisson_block(6, 6, 6)
    b = synthetic.rhs_for_x_star(case)[0]
    s = reg.solver("mx_off_%s" % setting, cfg(adapt_min_iter=0)).set_matrix(case)
    if setting is not None:
        s.set_property("mixedPrecision", setting)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("mixedPrecisionInUse") == 0.0
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    with blocked(oracle, chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), oracle.jacobi_generate_scalar(rp, cols, vals), tolerance=1e-10, rel_tol=0.0,
                        max_iter=1000)
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)


# ---- 5. a time-step loop ----
def test_time_steps_follow_the_coefficients_and_stop_allocating(reg, oracle):
    s = reg.solver("mx_steps", cfg())
    s.set_mixed_precision(True)
    marks = {}
    x = np.zeros(630)  # (updateInitGuess 0, the default: every step starts from the solution of the step before)
    for step in range(4):
        case = randomise(synthetic.poisson_block(10, 9, 7), 40 + step)
        b = np.random.default_rng(50 + step).uniform(-1, 1, case.n_cells)
        s.set_matrix(case)
        rp, cols, vals = oracle_csr(oracle, case)
        with blocked(oracle, chunk_rows()):
            w = mw.mixed_walk(oracle, rp, cols, vals, b, x, oracle.jacobi_generate_scalar(rp, cols, vals),
                              tolerance=1e-10, rel_tol=0.0)
        x, perf = s.solve(b, x)
        print("step", step, perf.n_iterations, s.get_property("mixedOuterSteps"), "walk:", w.n_iterations, w.outer_steps)
        assert w.smallest_fp32 >= mw.TINY32 and w.outer_steps >= 2
        assert (perf.n_iterations, s.get_property("mixedOuterSteps")) == (w.n_iterations, w.outer_steps)
        np.testing.assert_array_equal(s.history(), w.history)
        np.testing.assert_array_equal(x, w.x)
        marks[step] = capi.memory_ledger().as_dict()
    for k in ("device_alloc_calls", "pinned_alloc_calls", "device_bytes", "pinned_bytes"):
        assert marks[3][k] == marks[1][k], (k, marks)
