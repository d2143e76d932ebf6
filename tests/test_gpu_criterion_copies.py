"""Every caller of the stopping criterion (StoppingCriterion.C:71-151) and every breakdown guard of the Krylov loop, on every
turn shape that carries one, bit for bit against the oracle run in the device's reduction tree.

The criterion is written out once, in criterion_verdict (device_common.hpp); what each kernel does around the verdict is
its own: k_finalize (through criterion_check), k_cg_step1x_fin, k_bicg_fold1, k_bicg_fold3 (kernels_krylov.hip),
k_cg_turn_sym (kernels_spmv_sym.hip) and the resident turn body (resident_cg_turn.hpp) that k_cg_step2r1x and
k_cg_turn_held_q run; Ginkgo's zero guards
(prev_rho == 0, beta != 0, prev_rho * omega != 0, omega's v1 != 0, H(it, it) == 0) in each step kernel and finaliser.
SHAPES names the properties that force each turn shape and the properties that prove it ran; both are set and asserted
in every solve.  One handle per shape: the configuration changes between solves, the handle stays.

Section 2 (test_criterion_*): the stop positions come from a probe run of the oracle (tolerance 0), never from a
constant: T(k) = nextafter(h[k], inf) for a record low h[k] is first met at check k.  stops_at states where a case is
MEANT to stop, the oracle must agree with it, and the bits come from the oracle.  Section 3 (test_degenerate_*): inputs
that are exact in binary floating point, so the expected values are closed forms as well as oracle output; a NaN that
the reference produces (it divides r by its zero norm) is arithmetic, the solve returns normally and the next solve
on the same handle is the oracle's again."""
import dataclasses
from collections import namedtuple

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_matrix

pytestmark = pytest.mark.gpu

CHUNK = 512
CG, BICG, GMRES = capi.SOLVER_CG, capi.SOLVER_BICGSTAB, capi.SOLVER_GMRES
BOX = {"S": (14, 14, 14), "L": (30, 30, 28)}        # 2,744 rows = 6 chunks; 25,200 rows = 50 chunks
LINE = {"S": 3 * CHUNK + 5, "L": 48 * CHUNK + 1}    # 4 chunks; 49 chunks, the last one of one row
PROBE_ITERS = {CG: 30, BICG: 30, GMRES: 40}
KRYLOV_DIM = 5
HUGE = 2.0 ** 600   # exact; its square is past the largest double
LAST = 30    # the check every criterion case stops at at the latest: a multiple of evalFrequency 1, 2 and 3

Shape = namedtuple("Shape", "solver size props expect")
System = namedtuple("System", "key case b A csr inv precond")
Out = namedtuple("Out", "x n_iterations n_norm_evals history initial_residual final_residual norm_factor")


def _p(**kw):
    return tuple((k, float(v)) for k, v in kw.items())


LEAD = dict(fusedFinMaxChunks=0)   # no fused finalisers at any size: the leader turn from 48 chunks on
SHAPES = {
    # GKOCG
    "cg-five-S": Shape(CG, "S", _p(fusedFinalizers=0, leadFinalizers=0, fusedTurnBig=0),
                       _p(fusedFinalizersInUse=0, leadFinalizersInUse=0, fusedTurnInUse=0)),
    "cg-five-L": Shape(CG, "L", _p(fusedFinalizers=0, leadFinalizers=0, fusedTurnBig=0),
                       _p(fusedFinalizersInUse=0, leadFinalizersInUse=0, fusedTurnInUse=0)),
    "cg-merged-S": Shape(CG, "S", _p(fusedFinalizers=0, leadFinalizers=0, fusedTurnBig=1),
                         _p(fusedFinalizersInUse=0, leadFinalizersInUse=0, fusedTurnInUse=1)),
    "cg-small3-S": Shape(CG, "S", _p(fusedTurn=0), _p(fusedFinalizersInUse=1, leadFinalizersInUse=0, fusedTurnInUse=0)),
    "cg-small2-S": Shape(CG, "S", (), _p(fusedFinalizersInUse=1, leadFinalizersInUse=0, fusedTurnInUse=1)),
    "cg-lead3-d0-L": Shape(CG, "L", _p(fusedTurnBig=0, heldZ=0, deferX=0, **LEAD),
                           _p(leadFinalizersInUse=1, fusedFinalizersInUse=0, fusedTurnInUse=0, heldZInUse=0, deferXInUse=0)),
    "cg-lead3-d2-L": Shape(CG, "L", _p(fusedTurnBig=0, heldZ=0, deferX=2, **LEAD),
                           _p(leadFinalizersInUse=1, fusedFinalizersInUse=0, fusedTurnInUse=0, heldZInUse=0, deferXInUse=2)),
    "cg-lead2-L": Shape(CG, "L", _p(fusedTurnBig=1, **LEAD),
                        _p(leadFinalizersInUse=1, fusedFinalizersInUse=0, fusedTurnInUse=1)),
    # GKOBiCGStab
    "bicg-own-S": Shape(BICG, "S", _p(bicgFold=0, bicgMergedCheck=0), _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "bicg-own-L": Shape(BICG, "L", _p(bicgFold=0, bicgMergedCheck=0, **LEAD),
                        _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "bicg-merged-S": Shape(BICG, "S", _p(bicgFold=0, bicgMergedCheck=1), _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "bicg-merged-L": Shape(BICG, "L", _p(bicgFold=0, bicgMergedCheck=1, **LEAD),
                           _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "bicg-fold-S": Shape(BICG, "S", (), _p(fusedFinalizersInUse=1, leadFinalizersInUse=0)),
    "bicg-lead-L": Shape(BICG, "L", _p(**LEAD), _p(leadFinalizersInUse=1, fusedFinalizersInUse=0)),
    # GKOGMRES
    "gmres-own-S": Shape(GMRES, "S", _p(gmresFold=0), _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "gmres-own-L": Shape(GMRES, "L", _p(gmresFold=0, **LEAD), _p(fusedFinalizersInUse=0, leadFinalizersInUse=0)),
    "gmres-fold-S": Shape(GMRES, "S", (), _p(fusedFinalizersInUse=1, leadFinalizersInUse=0)),
    "gmres-lead-L": Shape(GMRES, "L", _p(gmresLead=1, **LEAD), _p(leadFinalizersInUse=1, fusedFinalizersInUse=0)),
}
# the held-z turn: its criterion matrix is pinned in test_gpu_held_z_load.py, its guards here (section 3 only)
HELD = {
    "cg-heldz-d0-L": Shape(CG, "L", _p(fusedTurnBig=0, heldZ=1, deferX=0, **LEAD),
                           _p(leadFinalizersInUse=1, fusedTurnInUse=0, heldZInUse=1, deferXInUse=0)),
    "cg-heldz-d2-L": Shape(CG, "L", _p(fusedTurnBig=0, heldZ=1, deferX=2, **LEAD),
                           _p(leadFinalizersInUse=1, fusedTurnInUse=0, heldZInUse=1, deferXInUse=2)),
}
ALL_SHAPES = {**SHAPES, **HELD}


_systems = {}   # key -> System: the pattern, the oracle's matrix and preconditioner, once per system
_refs = {}      # (system, solver, right-hand side, start vector, criterion) -> oracle result, never changed


@pytest.fixture(scope="module", autouse=True)
def oracle_cache():
    """The oracle's systems and results live as long as this module's tests."""
    yield
    _systems.clear()
    _refs.clear()


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def make_system(oracle, key, case, b=None):
    if key not in _systems:
        A, csr = oracle_matrix(oracle, case)
        b = synthetic.rhs_for_x_star(case)[0] if b is None else b(csr)
        _systems[key] = System(key, case, b, A, csr, oracle.jacobi_generate_scalar(*csr), oracle.Precond(*csr, 1))
    return _systems[key]


def box(oracle, solver, size):
    """The symmetric box for GKOCG, upper -0.9 / lower -1.1 for the other two; b = A x*."""
    kw = {} if solver == CG else dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
    return make_system(oracle, ("box", solver == CG, size), synthetic.poisson_block(*BOX[size], **kw))


def reference(oracle, sy, solver, crit, precond=True, b=None, x0=None, tag=None):
    """The oracle in the device's reduction tree, once per (system, right-hand side, start vector, criterion)."""
    key = (sy.key, solver, precond, tag, tuple(sorted(crit.items())))
    if key not in _refs:
        b = sy.b if b is None else b
        x0 = np.zeros_like(b) if x0 is None else x0
        with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
            if solver == GMRES:
                _refs[key] = oracle.gmres(sy.A, b, x0, sy.precond if precond else None, **crit)
            else:
                fn = oracle.cg if solver == CG else oracle.bicgstab
                _refs[key] = fn(sy.A, b, x0, sy.inv if precond else None, **crit)
    return _refs[key]


def solve(reg, name, handle, sy, crit, precond=True, b=None, x0=None, export_res=1):
    """One solve of shape `name` on the handle `handle`: forces the shape, asserts the properties that prove it ran."""
    shape = ALL_SHAPES[name]
    kw = dict(crit)
    if "frequency" in kw:
        kw["eval_frequency"] = kw.pop("frequency")
    cfg = capi.default_config(solver=shape.solver, export_res=export_res, adapt_min_iter=0, update_init_guess=1,
                              preconditioner=capi.PRECOND_BJ if precond else capi.PRECOND_NONE, **kw)
    s = reg.solver(handle, cfg)
    for k, v in shape.props:
        s.set_property(k, v)
    s.set_matrix(sy.case)
    b = sy.b if b is None else b
    x, perf = s.solve(b, np.zeros_like(b) if x0 is None else x0)
    for k, v in shape.expect:
        assert s.get_property(k) == v, (name, k, s.get_property(k))
    return Out(x, perf.n_iterations, perf.n_norm_evals, s.history().copy(), perf.initial_residual, perf.final_residual, perf.norm_factor)


def assert_scalars(out, ref, solver):
    assert out.n_iterations == (ref.n_iterations // 2 if solver == BICG else ref.n_iterations)
    assert out.n_norm_evals == ref.n_evals
    for name in ("initial_residual", "final_residual", "norm_factor"):   # (array_equal: NaN equals NaN)
        np.testing.assert_array_equal(getattr(out, name), getattr(ref, name), err_msg=name)


def assert_oracle(out, ref, solver):
    assert_scalars(out, ref, solver)
    np.testing.assert_array_equal(out.history, ref.history)
    np.testing.assert_array_equal(out.x, ref.x)


# ---- section 2: the criterion matrix ----
def stops_at(h, tolerance=0.0, rel_tol=0.0, min_iter=0, max_iter=600, frequency=1):
    """The check at which the criterion stops a run whose residuals are h (StoppingCriterion semantics: no verdict below
    min_iter nor off the frequency).  Used only to state where a case is MEANT to stop; the bits come from the oracle."""
    for k in range(len(h)):
        if (0 < k < min_iter) or k % frequency:
            continue
        if k >= max_iter or h[k] < tolerance or (rel_tol > 0 and h[k] < rel_tol * h[0]):
            return k
    raise AssertionError("no stop inside the probe")


def solver_kw(solver):
    return dict(krylov_dim=KRYLOV_DIM) if solver == GMRES else {}


def probe(oracle, sy, solver):
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=PROBE_ITERS[solver], **solver_kw(solver))
    h = reference(oracle, sy, solver, crit).history
    assert h.size == (2 if solver == BICG else 1) * PROBE_ITERS[solver] + 1 and np.all(h > 0.0)
    return h


def record_lows(h):
    return [k for k in range(1, len(h)) if h[k] < h[:k].min()]


def pick(solver, h):
    """(ka, kb): two record lows of the probe.  GKOBiCGStab: ka even (the check at the head of a turn), kb odd (the
    mid-turn check on s).  GKOGMRES(5): the checks that first see the residual of the first and second restart."""
    lows = record_lows(h)
    if solver == GMRES:
        assert lows[:2] == [KRYLOV_DIM + 1, 2 * KRYLOV_DIM + 1], lows
        return lows[0], lows[1]
    if solver == BICG:
        ka = min(k for k in lows if k >= 10 and k % 2 == 0)
        kb = min(k for k in lows if k >= 9 and k % 2 == 1)
    else:
        ka = min(k for k in lows if k >= 5)
        kb = min(k for k in lows if k >= ka + 3)
    assert max(ka, kb) + 2 < LAST - 6, (ka, kb)
    return ka, kb


MIN_ITER_CASES = [f"min-{which}{d:+d}-f{f}" for which in ("ka", "kb") for d in (-1, 0, 1, 2) for f in (1, 2, 3)]
COMMON_CASES = (["tol-ka", "tol-kb", "tol-ka-f2", "tol-ka-f3", "tol-kb-f2", "tol-kb-f3", "strict-ka", "strict-kb", "rel-ka",
                 "rel-kb", "tol-before-rel", "rel-before-tol"] + MIN_ITER_CASES +
                ["max-no-multiple-f3", "min-above-max-f1", "min-above-max-f2", "max-0"])
GMRES_CASES = ["max-5-f2", "max-6-f2", "max-7-f2"]
# cases whose stop the tolerance decides (at the check in the name when min_iter and the frequency let it look there)
EXPORT_OFF_CASES = ["tol-ka", "tol-kb", "rel-kb", "min-ka+1-f2", "min-kb+2-f3", "max-no-multiple-f3", "min-above-max-f2", "max-0"]


def criteria(solver, h):
    """name -> (criterion as the keywords give it, the check it is built to stop at or None where only `later than k`
    is built in, the k it is later than).  max_iter is the keyword: GKOBiCGStab doubles it."""
    ka, kb = pick(solver, h)
    lo, hi = min(ka, kb), max(ka, kb)
    per_iter = 2 if solver == BICG else 1     # checks per unit of maxIter
    last = LAST // per_iter

    def T(k):
        assert h[k] < h[:k].min()
        return float(np.nextafter(h[k], np.inf))

    def rel(k):   # half way between the record low and the lowest value before it, relative to the first residual
        assert h[k] < h[:k].min()
        return 0.5 * float(h[k] + h[:k].min()) / float(h[0])

    out = {}
    for name, k in (("ka", ka), ("kb", kb)):
        out[f"tol-{name}"] = (dict(tolerance=T(k), rel_tol=0.0, max_iter=last), k, None)
        for f in (2, 3):   # first met at k; stops at the first evaluated check from k on that is below it
            out[f"tol-{name}-f{f}"] = (dict(tolerance=T(k), rel_tol=0.0, max_iter=last, frequency=f), None, k - 1)
        # res < tolerance is strict: h[k] itself does not stop at k
        out[f"strict-{name}"] = (dict(tolerance=float(h[k]), rel_tol=0.0, max_iter=last), None, k)
        out[f"rel-{name}"] = (dict(tolerance=0.0, rel_tol=rel(k), max_iter=last), k, None)
        for d in (-1, 0, 1, 2):
            for f in (1, 2, 3):
                out[f"min-{name}{d:+d}-f{f}"] = (dict(tolerance=T(k), rel_tol=0.0, min_iter=k + d, max_iter=last, frequency=f),
                                                 None, max(k, k + d) - 1)
    out["tol-before-rel"] = (dict(tolerance=T(lo), rel_tol=rel(hi), max_iter=last), lo, None)
    out["rel-before-tol"] = (dict(tolerance=T(hi), rel_tol=rel(lo), max_iter=last), lo, None)
    # 7 (GKOBiCGStab: 2 x 4 = 8) is no multiple of 3: the first evaluated check at or after it is 9, a mid-turn check
    out["max-no-multiple-f3"] = (dict(tolerance=0.0, rel_tol=0.0, max_iter=4 if solver == BICG else 7, frequency=3), 9, None)
    # min_iter above max_iter (5; GKOBiCGStab: 2 x 3 = 6): no verdict below min_iter, the run goes on to it
    small = 3 if solver == BICG else 5
    out["min-above-max-f1"] = (dict(tolerance=0.0, rel_tol=0.0, min_iter=9, max_iter=small), 9, None)
    out["min-above-max-f2"] = (dict(tolerance=0.0, rel_tol=0.0, min_iter=9, max_iter=small, frequency=2), 10, None)
    out["max-0"] = (dict(tolerance=0.0, rel_tol=0.0, max_iter=0), 0, None)
    if solver == GMRES:   # the evaluated checks and the restart (after check 5) interleave
        for m, stop in ((5, 6), (6, 6), (7, 8)):
            out[f"max-{m}-f2"] = (dict(tolerance=0.0, rel_tol=0.0, max_iter=m, frequency=2), stop, None)
    return {k: ({**c, **solver_kw(solver)}, at, after) for k, (c, at, after) in out.items()}


def expected(oracle, sy, solver, which):
    """(criterion, oracle result) of case `which`: the oracle stops where stops_at says, and that is where the case is
    built to stop."""
    h = probe(oracle, sy, solver)
    crit, at, after = criteria(solver, h)[which]
    model = {k: v for k, v in crit.items() if k != "krylov_dim"}
    if solver == BICG:
        model["max_iter"] = 2 * model["max_iter"]
    stop = stops_at(h, **model)
    assert (stop == at) if at is not None else (stop > after), (which, stop, at, after)
    if which.split("-")[0] in ("tol", "strict", "rel") or (which.startswith("min-k")):
        assert stop < LAST, (which, stop)   # (the bound decides, not max_iter)
    ref = reference(oracle, sy, solver, crit)
    assert ref.n_iterations == stop + 1, (which, ref.n_iterations, stop)
    np.testing.assert_array_equal(ref.history[ref.history != 0.0], h[:stop + 1][ref.history != 0.0])
    return crit, ref


def cases_of(solver):
    return COMMON_CASES + (GMRES_CASES if solver == GMRES else [])


def criterion_params():
    return [pytest.param(name, which, id=f"{name}-{which}") for name, shape in SHAPES.items() for which in cases_of(shape.solver)]


@pytest.mark.parametrize("name,which", criterion_params())
def test_criterion_on_every_shape(reg, oracle, name, which):
    """tolerance, its strictness, rel_tol, both together, min_iter around the stop at evalFrequency 1, 2 and 3, a max_iter
    that is no multiple of the frequency, min_iter above max_iter and max_iter 0: history, x, both counters, both
    residuals and the norm factor are the oracle's."""
    shape = SHAPES[name]
    sy = box(oracle, shape.solver, shape.size)
    crit, ref = expected(oracle, sy, shape.solver, which)
    assert_oracle(solve(reg, name, name, sy, crit), ref, shape.solver)


@pytest.mark.parametrize("name", [n for n, s in SHAPES.items() if s.solver == BICG])
def test_both_stop_positions_are_covered(oracle, name):
    """Every GKOBiCGStab shape above stops by a bound at the head of a turn (even check: x is up to date) and in mid-turn
    (odd check: bicgstab::finalize, x += alpha y), with evalFrequency 1 and 3; with evalFrequency 2 the mid-turn check
    never evaluates and every stop is even."""
    shape = SHAPES[name]
    sy = box(oracle, BICG, shape.size)
    seen = {1: set(), 2: set(), 3: set()}
    for which in COMMON_CASES:
        crit, ref = expected(oracle, sy, BICG, which)
        if crit["tolerance"] > 0.0 or crit["rel_tol"] > 0.0:
            assert ref.n_iterations - 1 < LAST
            seen[crit.get("frequency", 1)].add((ref.n_iterations - 1) % 2)
    assert seen == {1: {0, 1}, 2: {0}, 3: {0, 1}}


@pytest.mark.parametrize("name", list(SHAPES))
def test_criterion_without_exported_residuals(reg, oracle, name):
    """export_res 0: x, both counters and both residuals are those of the export_res 1 run on the same handle, and the
    oracle's, and no history comes back.  (Whether a kernel's c_exp branch stores a residual cannot be seen from
    outside: the device history is read back only with export_res 1, after it was zeroed at that solve's start.)"""
    shape = SHAPES[name]
    sy = box(oracle, shape.solver, shape.size)
    for which in EXPORT_OFF_CASES:
        crit, ref = expected(oracle, sy, shape.solver, which)
        off = solve(reg, name, name, sy, crit, export_res=0)
        on = solve(reg, name, name, sy, crit, export_res=1)
        assert_oracle(on, ref, shape.solver)
        assert_scalars(off, ref, shape.solver)
        np.testing.assert_array_equal(off.x, ref.x)
        assert off.history.size == 0
        assert (off.n_iterations, off.n_norm_evals, off.initial_residual, off.final_residual) == \
               (on.n_iterations, on.n_norm_evals, on.initial_residual, on.final_residual), which


# ---- section 3: breakdown and degenerate inputs ----
def line(oracle, solver, size, kind):
    """kind "dyadic": diagonal 2.5, off-diagonals -1 (every product with a small integer is exact).  kind "diagonal":
    off-diagonals 0 with the pattern kept, diagonal +1 except -1 at rows 512 and n - 1; b = 1 at rows 510, 511, 512 and
    n - 1: r . A r = 2 - 2 = 0 exactly.  kind "hollow": diagonal 0, off-diagonals 2^600; b = 1 at row 511: A r is
    orthogonal to r and its square overflows.  GKOBiCGStab and GKOGMRES get `lower` as an array of its own."""
    n = LINE[size]
    kw = {} if solver == CG else dict(symmetric=False)
    case = synthetic.poisson_block(n, 1, 1, **kw)
    off = {"dyadic": -1.0, "diagonal": 0.0, "hollow": HUGE}[kind]
    diag = {"dyadic": np.full(n, 2.5), "diagonal": np.ones(n), "hollow": np.zeros(n)}[kind]
    if kind == "diagonal":
        diag[[512, n - 1]] = -1.0
    case = dataclasses.replace(case, diag=diag, upper=np.full_like(case.upper, off),
                               lower=None if case.lower is None else np.full_like(case.lower, off))

    def rhs(csr):
        b = np.zeros(n)
        if kind == "diagonal":
            b[[510, 511, 512, n - 1]] = 1.0
        if kind == "hollow":
            b[511] = 1.0
        return b

    return make_system(oracle, ("line", solver == CG, size, kind), case, rhs)


def after_degenerate(reg, oracle, name, handle):
    """(d) the same handle on the ordinary box of its shape, with a criterion of section 2: nothing of the solve before
    -- a NaN in the p ring, the leader mailbox, DevScalars or the GMRES state -- outlives it."""
    shape = ALL_SHAPES[name]
    sy = box(oracle, shape.solver, shape.size)
    crit, ref = expected(oracle, sy, shape.solver, "tol-kb")
    assert_oracle(solve(reg, name, handle, sy, crit), ref, shape.solver)


def degenerate(reg, oracle, name, handle, sy, crit, tag, **kw):
    shape = ALL_SHAPES[name]
    crit = {**solver_kw(shape.solver), **crit}
    ref = reference(oracle, sy, shape.solver, crit, tag=tag, **kw)
    out = solve(reg, name, handle, sy, crit, **kw)
    assert_oracle(out, ref, shape.solver)
    return out


def checks(solver, max_iter):
    return 2 * max_iter + 1 if solver == BICG else max_iter + 1


@pytest.mark.parametrize("precond", [True, False], ids=["BJ", "none"])
@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_degenerate_exact_start_vector(reg, oracle, name, precond):
    """(a) x0 = x*, b = A x* by the oracle's row loop, x* small integers: r = 0 exactly.  GKOCG: rho = 0, p.q = 0, no step.
    GKOBiCGStab: alpha's, omega's and step_1's guards all see zeros.  GKOGMRES stops at check 0 when a tolerance lets it;
    with tolerance 0 the reference divides r by its zero norm: history [0, 0, 0, nan] with krylov_dim 2, x all NaN, and
    the solve returns normally."""
    shape = ALL_SHAPES[name]
    sy = line(oracle, shape.solver, shape.size, "dyadic")
    handle = f"{name}_deg_{precond}"
    xs = np.random.default_rng(LINE[shape.size]).integers(-8, 9, sy.case.n_cells).astype(np.float64)
    b = oracle.spmv(*sy.csr, xs)
    kw = dict(precond=precond, b=b, x0=xs)
    if shape.solver == GMRES:
        out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=1e-6, rel_tol=0.0, max_iter=3), "exact", **kw)
        assert out.n_iterations == 1
        np.testing.assert_array_equal(out.history, [0.0])
        np.testing.assert_array_equal(out.x, xs)
        out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=3, krylov_dim=2), "exact", **kw)
        np.testing.assert_array_equal(out.history, [0.0, 0.0, 0.0, np.nan])
        assert np.isnan(out.x).all()
    else:
        out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=3), "exact", **kw)
        assert out.n_iterations == (4 if shape.solver == CG else 7 // 2)
        np.testing.assert_array_equal(out.history, np.zeros(checks(shape.solver, 3)))
        np.testing.assert_array_equal(out.x, xs)
    after_degenerate(reg, oracle, name, handle)


@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_degenerate_zero_right_hand_side(reg, oracle, name):
    """(b) b = 0, x0 = 0: the norm factor is the SMALL it ends with, 1e-15; a tolerance stops at check 0; without one
    GKOCG and GKOBiCGStab run to max_iter on zeros."""
    shape = ALL_SHAPES[name]
    sy = line(oracle, shape.solver, shape.size, "dyadic")
    handle = f"{name}_deg_True"
    out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=1e-6, rel_tol=0.0, max_iter=3), "zero")
    assert out.norm_factor == 1e-15 and out.n_norm_evals == 1
    np.testing.assert_array_equal(out.history, [0.0])
    np.testing.assert_array_equal(out.x, np.zeros(sy.case.n_cells))
    if shape.solver != GMRES:
        out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=3), "zero")
        assert out.norm_factor == 1e-15
        np.testing.assert_array_equal(out.history, np.zeros(checks(shape.solver, 3)))
        np.testing.assert_array_equal(out.x, np.zeros(sy.case.n_cells))
    after_degenerate(reg, oracle, name, handle)


@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_degenerate_breakdown_in_mid_solve(reg, oracle, name):
    """(c) r . A r = 0 with r != 0, no preconditioner, tolerance 0.  GKOCG: p.q == 0, no step, beta 0.  GKOBiCGStab:
    rr.v == 0 gives alpha 0, s.t == 0 gives omega 0, and step_1's prev_rho * omega guard fires on every later turn.
    GKOGMRES(5): H(0,0) == 0 takes the c = 0, s = 1 branch, the second column closes the Krylov space (hn == 0): two
    columns give A^-1 b, one gives 0, three and four divide by hn and make every entry of x NaN.  The history is
    constant at 4 / norm_factor throughout."""
    shape = ALL_SHAPES[name]
    sy = line(oracle, shape.solver, shape.size, "diagonal")
    n = sy.case.n_cells
    handle = f"{name}_deg_False"
    zero = np.zeros(n)
    for max_iter in ((3,) if shape.solver != GMRES else (1, 2, 3, 4)):
        out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=max_iter), "breakdown",
                         precond=False)
        assert out.norm_factor == 4.000000000000001
        np.testing.assert_array_equal(out.history, np.full(checks(shape.solver, max_iter), 4.0 / out.norm_factor))
        if shape.solver != GMRES or max_iter == 1:
            np.testing.assert_array_equal(out.x, zero)
        elif max_iter == 2:
            inverse = zero.copy()
            inverse[[510, 511]] = 1.0
            inverse[[512, n - 1]] = -1.0
            np.testing.assert_array_equal(out.x, inverse)
        else:
            assert np.isnan(out.x).all()
            after_degenerate(reg, oracle, name, handle)   # (d) right after each solve that left NaN behind
    if not np.isnan(out.x).any():
        after_degenerate(reg, oracle, name, handle)


@pytest.mark.parametrize("name", [n for n, s in SHAPES.items() if s.solver == GMRES])
def test_degenerate_zero_pivot_of_the_givens_rotation(reg, oracle, name):
    """The H(it, it) == 0 branch of givens_rotation where it decides the result.  With a finite hn the general branch
    gives c = 0, s = 1 as well (scale = hn, a0 = 0, a1 = 1, hyp = hn, exactly), and with hn == 0 the triangular solve
    divides 0 by 0 either way; the branch is the only way to a finite x when hn is infinite.  Diagonal 0, off-diagonals
    2^600, b = e_511, no preconditioner: V_0 = b, w = A V_0 is 2^600 at rows 510 and 512 (two chunks), H(0,0) = w . V_0
    = 0, hn = sqrt(2^1201) = inf.  The branch gives c = 0, s = 1, H(0,0) = inf, the residual norm vector (0, -1), so one
    column gives y = 0 / inf = 0 and x = 0 exactly; the general branch would divide inf by inf.  V_1 = w / inf = 0, so
    the second column is 0 / 0 and every entry of x is NaN, as in the oracle.  The history sees the restart's norm only."""
    shape = SHAPES[name]
    sy = line(oracle, GMRES, shape.size, "hollow")
    handle = f"{name}_deg_False"
    out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=1), "hollow", precond=False)
    assert out.norm_factor == 1.000000000000001
    np.testing.assert_array_equal(out.history, np.full(2, 1.0 / out.norm_factor))
    np.testing.assert_array_equal(out.x, np.zeros(sy.case.n_cells))
    out = degenerate(reg, oracle, name, handle, sy, dict(tolerance=0.0, rel_tol=0.0, max_iter=2), "hollow", precond=False)
    np.testing.assert_array_equal(out.history, np.full(3, 1.0 / out.norm_factor))
    assert np.isnan(out.x).all()
    after_degenerate(reg, oracle, name, handle)
