"""The resident CG turn's head (resident_cg_turn.hpp, turn_phase_h): early x by slot count.

heldZEarlySlots k: a head that updates x writes x of its first k slots while rho and sum |r'| are awaited (a second read of
their p) and x of the other slots in the loop that forms p_new, from that loop's one read of p.  heldZEarlyX 0 still switches
early x off whatever the count.  The place of a slot's x update changes no bit: history, x, iteration count, final residual
and the number of norm evaluations are those of the two-launch turn (heldQ 0) at the default count, of the three-launch turn
(heldZ 0) and of the oracle in the device's reduction order -- for the one-launch kernel (k_cg_turn_held_q) and for the
held-z kernel (k_cg_step2r1x), which run the same body.

84^3 on 59 workgroups, as in tests/test_gpu_held_q.py: 55 workgroups own 20 positions, so every register slot (11) and every
LDS slot (9) is loaded; the counts are none, one, all register slots, one LDS slot more, and all.  With deferX 2 two
consecutive stops by maxIter fall on a deferring head (which writes what is pending in its last loop) and on one that updates
x.

The file's name comes from the work it was planned for: sum leaders that own no chunk.  They are not built and nothing here
tests them -- the time line of the two waits (profiles/r11_resident_waits.txt, section 2) left them nothing to gain."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_matrix

pytestmark = pytest.mark.gpu
N = 84
GRID = 59   # 55 workgroups own 20 positions, 4 own 19


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def make_system(oracle, case):
    b = synthetic.rhs_for_x_star(case)[0]
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    return case, b, A, oracle.jacobi_generate_scalar(rp, cols, vals)


@pytest.fixture(scope="module")
def system(oracle):
    return make_system(oracle, synthetic.poisson_case(N))


@pytest.fixture(scope="module")
def refs():
    """What the other turns and the oracle give, computed once per configuration and left unchanged."""
    return {}


_serial = [0]


def solver(reg, name, case, held_q, held_z=1.0, defer=2.0, grid=GRID, props=(), **kw):
    cfg = capi.default_config(solver=capi.SOLVER_CG, export_res=1, adapt_min_iter=0, update_init_guess=1, **kw)
    _serial[0] += 1  # (the registry looks solvers up by name: every construction here is a new one)
    s = reg.solver(f"{name}_{_serial[0]}", cfg)
    s.set_property("fusedTurnBig", 0.0)  # (the leader turn of three launches: what the resident turns replace)
    s.set_property("heldZ", held_z)
    s.set_property("heldQ", held_q)
    s.set_property("deferX", defer)
    if grid:
        s.set_property("heldZGrid", float(grid))
    for key, v in props:
        s.set_property(key, v)
    return s.set_matrix(case)


def solve(s, b, held_q, held_z=1.0, defer=2.0, x0=None):
    x, perf = s.solve(b, np.zeros_like(b) if x0 is None else x0)
    assert s.get_property("heldQInUse") == held_q and s.get_property("heldZInUse") == held_z
    assert s.get_property("leadFinalizersInUse") == 1.0 and s.get_property("fusedTurnInUse") == 0.0
    assert s.get_property("deferXInUse") == defer
    return x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals


def assert_same(a, b):
    assert a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])


def others(reg, oracle, refs, key, sysm, defer, grid, props=(), x0=None, **kw):
    """The two-launch turn (heldQ 0), the three-launch turn (heldZ 0) and the oracle's CG in the device's tree."""
    if key not in refs:
        case, b, A, inv = sysm
        two = solve(solver(reg, "rl_ref2", case, 0.0, 1.0, defer, grid, props, **kw), b, 0.0, 1.0, defer, x0)
        three = solve(solver(reg, "rl_ref3", case, 0.0, 0.0, defer, grid, props, **kw), b, 0.0, 0.0, defer, x0)
        okw = dict(tolerance=kw["tolerance"], rel_tol=kw["rel_tol"], max_iter=kw["max_iter"],
                   min_iter=kw.get("min_iter", 0), frequency=kw.get("eval_frequency", 1))
        with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
            ref = oracle.cg(A, b, np.zeros_like(b) if x0 is None else x0,
                            inv if kw["preconditioner"] == capi.PRECOND_BJ else None, **okw)
        refs[key] = (two, three, ref)
    return refs[key]


def assert_all_same(got, two, three, ref):
    assert_same(got, two)
    assert_same(got, three)
    assert ref.n_iterations == got[1]
    np.testing.assert_array_equal(got[2], ref.history)
    np.testing.assert_array_equal(got[0], ref.x)


SLOTS = [0.0, 1.0, 11.0, 12.0, 20.0]


@pytest.mark.parametrize("max_iter", [17, 18])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("slots", SLOTS)
def test_early_x_by_slot_count(reg, oracle, refs, system, slots, defer, max_iter):
    """The one-launch kernel."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    got = solve(solver(reg, "es_q", case, 1.0, 1.0, defer, props=(("heldZEarlySlots", slots),), **kw), b, 1.0, 1.0, defer)
    assert got[1] == max_iter + 1
    assert_all_same(got, *others(reg, oracle, refs, (capi.PRECOND_BJ, max_iter, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("max_iter", [17, 18])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("slots", SLOTS)
def test_early_x_by_slot_count_in_the_held_z_kernel(reg, oracle, refs, system, slots, defer, max_iter):
    """The two-launch turn: the stand-alone SpMV and the held-z kernel, whose slots are chunks w, w + 59, ..."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    got = solve(solver(reg, "es_z", case, 0.0, 1.0, defer, props=(("heldZEarlySlots", slots),), **kw), b, 0.0, 1.0, defer)
    assert_all_same(got, *others(reg, oracle, refs, (capi.PRECOND_BJ, max_iter, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("slots", [4.0, 20.0])
def test_early_x_off_whatever_the_count(reg, oracle, refs, system, slots, defer):
    """heldZEarlyX 0 wins over the count; without a preconditioner z is r' itself."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_NONE, tolerance=0.0, rel_tol=0.0, max_iter=18)
    props = (("heldZEarlySlots", slots), ("heldZEarlyX", 0.0))
    got = solve(solver(reg, "es_off", case, 1.0, 1.0, defer, props=props, **kw), b, 1.0, 1.0, defer)
    assert_all_same(got, *others(reg, oracle, refs, (capi.PRECOND_NONE, 18, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_a_count_beyond_the_slots_and_a_stop_by_tolerance(reg, oracle, refs, system, defer):
    """A count above R + L = 20 is clipped to it, a negative one to none; the stop comes from the criterion, with checks at
    every third turn."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=1e-2, rel_tol=0.0, max_iter=600, eval_frequency=3)
    want = others(reg, oracle, refs, ("tol", defer), system, defer, GRID, **kw)
    for slots in (64.0, -3.0, 6.0):
        got = solve(solver(reg, "es_tol", case, 1.0, 1.0, defer, props=(("heldZEarlySlots", slots),), **kw), b, 1.0, 1.0, defer)
        assert got[1] < 600 and got[1] % 3 == 1
        assert_all_same(got, *want)
