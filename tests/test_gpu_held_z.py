"""The held-z turn of single-rank GKOCG (kernels_krylov.hip, k_cg_step2r1x): step_2r of a turn and the head (check, pending
x update, step_1) of the next in one resident kernel that keeps z = r / d in registers and LDS across the grid-wide sums --
two launches per turn, SpMV | step_2r1x, instead of three.  The partials keep their tree, the sums the finaliser's, the
scalar logic is that of k_cg_step1x_fin: history, x, iteration count and final residual carry the bits of the three-launch
turn (heldZ 0) and of the oracle in the device's reduction order, wherever the criterion stops.

The default gate switches the turn on where the leader turn streams; the sizes here are far below that, so every test
forces it with the property and asserts heldZInUse.  heldZGrid lowers the number of resident workgroups, so that a small
system fills the register-held chunks of a workgroup (11) and spills over into its LDS-held ones."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_matrix

pytestmark = pytest.mark.gpu
N = 84        # 592,704 rows = 1,158 chunks (the leader turn's own size: tests/test_gpu_lead_finalizers.py)
GRID = 100    # 58 workgroups own 12 chunks (one of them in LDS), 42 own 11 (none in LDS)


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def make_system(oracle, n):
    case = synthetic.poisson_case(n)
    b = synthetic.rhs_for_x_star(case)[0]
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    return case, b, A, oracle.jacobi_generate_scalar(rp, cols, vals)


@pytest.fixture(scope="module")
def system(oracle):
    return make_system(oracle, N)


def solver(reg, name, case, held, defer=2.0, grid=GRID, props=(), **kw):
    cfg = capi.default_config(solver=capi.SOLVER_CG, export_res=1, adapt_min_iter=0, update_init_guess=1, **kw)
    s = reg.solver(name, cfg)
    s.set_property("fusedTurnBig", 0.0)  # (the leader turn of three launches: what the held-z turn replaces)
    s.set_property("heldZ", held)
    s.set_property("deferX", defer)
    if grid:
        s.set_property("heldZGrid", float(grid))
    for key, v in props:
        s.set_property(key, v)
    return s.set_matrix(case)


def solve(s, b, held, defer, x0=None):
    x, perf = s.solve(b, np.zeros_like(b) if x0 is None else x0)
    assert s.get_property("heldZInUse") == held
    assert s.get_property("leadFinalizersInUse") == 1.0 and s.get_property("fusedTurnInUse") == 0.0
    assert s.get_property("deferXInUse") == defer
    return x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals


def assert_same(a, b):
    assert a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("max_iter", [1, 2, 16, 17, 33, 60])
def test_same_bits_wherever_max_iter_stops(reg, oracle, system, precond, max_iter, defer):
    """Stops in every batch of 16 turns and at both ring positions."""
    case, b, A, inv = system
    kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    out = {h: solve(solver(reg, f"hz_{precond}_{defer}_{h}", case, h, defer, **kw), b, h, defer) for h in (1.0, 0.0)}
    assert out[1.0][1] == max_iter + 1
    assert_same(out[1.0], out[0.0])
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), inv if precond else None, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    assert ref.n_iterations == out[1.0][1]
    np.testing.assert_array_equal(out[1.0][2], ref.history)
    np.testing.assert_array_equal(out[1.0][0], ref.x)


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("tol", [1e-2, 1e-5, 1e-9])
def test_stop_by_tolerance_and_frequency(reg, oracle, system, tol, defer):
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=tol, rel_tol=0.0, max_iter=600, eval_frequency=3)
    out = {h: solve(solver(reg, f"hz_tol_{defer}_{h}", case, h, defer, **kw), b, h, defer) for h in (1.0, 0.0)}
    assert_same(out[1.0], out[0.0])
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), inv, tolerance=tol, rel_tol=0.0, max_iter=600, frequency=3)
    assert ref.n_iterations == out[1.0][1]
    np.testing.assert_array_equal(out[1.0][2], ref.history)
    np.testing.assert_array_equal(out[1.0][0], ref.x)


def test_a_second_solve_and_a_converged_guess(reg, system):
    """The tagged partials are cleared and the tags restart with every solve; a guess that already satisfies the
    criterion stops at the first (stand-alone) head, and the resident kernel that follows leaves everything alone."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=1e-8, rel_tol=0.0, max_iter=600)
    s = solver(reg, "hz_twice", case, 1.0, **kw)
    first = solve(s, b, 1.0, 2.0)
    second = solve(s, b, 1.0, 2.0)
    assert_same(first, second)
    assert_same(first, solve(solver(reg, "hz_twice_off", case, 0.0, **kw), b, 0.0, 2.0))
    third = solve(s, b, 1.0, 2.0, x0=first[0].copy())
    assert third[1] == 1
    np.testing.assert_array_equal(third[0], first[0])


@pytest.mark.parametrize("graph", [0.0, 1.0])
@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_graph_replay_on_and_off(reg, system, graph, defer):
    """Batches of 16 turns replayed from one captured graph (the first batch, with the stand-alone head, runs direct):
    the ring position of the head inside the kernel alternates exactly as the three-launch turn's."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=60)
    s = solver(reg, f"hz_graph_{graph}_{defer}", case, 1.0, defer, props=(("hipGraph", graph), ("hipGraphCaptures", 0.0)), **kw)
    got = solve(s, b, 1.0, defer)
    assert (s.get_property("hipGraphCaptures") >= 1.0) == (graph == 1.0)
    again = solve(s, b, 1.0, defer)  # (the second solve replays what the first has captured)
    assert_same(got, again)
    assert_same(got, solve(solver(reg, f"hz_graph_off_{graph}_{defer}", case, 0.0, defer, props=(("hipGraph", graph),), **kw),
                           b, 0.0, defer))


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("grid", [0, 32])
def test_partial_last_chunk(reg, oracle, precond, grid):
    """30^3 = 27,000 rows = 53 chunks, the last one of 376 rows (fusedFinMaxChunks 0 puts the leader turn on from 48
    chunks).  grid 0: the device's full resident grid, most of whose workgroups own no chunk; 32: the leaders alone, 21
    with two chunks and 11 with one."""
    case, b, A, inv = make_system(oracle, 30)
    kw = dict(preconditioner=precond, tolerance=1e-9, rel_tol=0.0, max_iter=300)
    props = (("fusedFinMaxChunks", 0.0),)
    out = {h: solve(solver(reg, f"hz_part_{precond}_{grid}_{h}", case, h, grid=grid, props=props, **kw), b, h, 2.0)
           for h in (1.0, 0.0)}
    assert_same(out[1.0], out[0.0])
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), inv if precond else None, tolerance=1e-9, rel_tol=0.0, max_iter=300)
    assert ref.n_iterations == out[1.0][1]
    np.testing.assert_array_equal(out[1.0][2], ref.history)
    np.testing.assert_array_equal(out[1.0][0], ref.x)


def test_full_grid_with_uneven_chunk_counts(reg, system):
    """1,158 chunks on the device's full resident grid: its first workgroups own two chunks, the others one."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=40)
    assert_same(solve(solver(reg, "hz_full_on", case, 1.0, grid=0, **kw), b, 1.0, 2.0),
                solve(solver(reg, "hz_full_off", case, 0.0, grid=0, **kw), b, 0.0, 2.0))


def test_above_the_cap_the_three_launch_turn_runs(reg, system):
    """heldZMaxChunks can only lower what the resident grid holds: one chunk below this system's 1,158 the held-z turn
    stays off although it is asked for, and the three-launch turn gives the same bits."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=40)
    on = solve(solver(reg, "hz_cap_fits", case, 1.0, props=(("heldZMaxChunks", 1158.0),), **kw), b, 1.0, 2.0)
    above = solve(solver(reg, "hz_cap_above", case, 1.0, props=(("heldZMaxChunks", 1157.0),), **kw), b, 0.0, 2.0)
    assert_same(on, above)
    # (... and without the property the grid's own capacity is the cap: 100 workgroups x 20 chunks hold 1,158, 57 do not)
    s = solver(reg, "hz_cap_grid", case, 1.0, grid=57, **kw)
    assert_same(on, solve(s, b, 0.0, 2.0))


@pytest.mark.parametrize("held", [1.0, 0.0])
def test_the_host_sees_the_stop_one_batch_late(reg, system, held):
    """The held-z turn leaves the scalars in the second slot, and that is the slot the host polls: it stops enqueuing at most
    two batches of 16 turns after the stop, as with the three-launch turn, instead of running on to max_iter."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=1e-5, rel_tol=0.0, max_iter=600)
    s = solver(reg, f"hz_poll_{held}", case, held, **kw)
    got = solve(s, b, held, 2.0)
    assert s.get_property("turnsEnqueued") <= got[1] + 2 * 16
