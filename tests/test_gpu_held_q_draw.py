"""Phase S of the held-q turn draws its positions (kernels_spmv_sym.hip, k_cg_turn_held_q; property heldQStaticSlots): slot
i < S of workgroup w holds position w + i G as before, the positions from S G on form eight queues (position p: queue p % 8)
and workgroup w takes the next of queue w % 8 for every further slot, up to 22 slots -- two more than the 20 the gates count.
Who computes a chunk changes nothing: partials and tagged words are per chunk, the row sums are k_spmv_sym's.  So every case
here carries the bits of the two-launch turn (heldQ 0), of the three-launch turn (heldZ 0) and of the oracle in the device's
reduction order, for every S, wherever the solve stops.

The helpers are those of test_gpu_held_q.py; the references never see the draw's properties and are computed once per
configuration."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked
from test_gpu_held_q import GRID, N, assert_all_same, assert_same, make_system, others, solve, solver

pytestmark = pytest.mark.gpu
SLOTS, GATE_SLOTS, XCDS = 22, 20, 8
FIN0 = (("fusedFinMaxChunks", 0.0),)  # (below 1,025 chunks every workgroup would reduce for itself: no leader turn)


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module")
def system(oracle):
    return make_system(oracle, synthetic.poisson_case(N))


@pytest.fixture(scope="module")
def refs():
    return {}


def drawn(static, idle=0.0):
    return (("heldQStaticSlots", float(static)), ("heldQIdleGroups", float(idle)))


def solve_drawn(s, b, in_use, defer=2.0, x0=None):
    got = solve(s, b, 1.0, 1.0, defer, x0)
    assert s.get_property("heldQStaticSlotsInUse") == in_use
    # (the static map runs the kernel with the gate's 20 slots, the draw the one with 22)
    assert s.get_property("heldQSlotsPerGroup") == (SLOTS if in_use < GATE_SLOTS else GATE_SLOTS)
    return got


@pytest.mark.parametrize("max_iter", [17, 33])
@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("static", [0, 1, 12, 19, 20])
def test_every_split_between_static_and_drawn_slots(reg, oracle, refs, system, static, defer, precond, max_iter):
    """84^3 on 59 workgroups: 1,158 chunks in 1,176 positions of a band order with holes, stops in two batches and at both
    ring positions.  59 is no multiple of 8: the queues have 7 or 8 workgroups, the draw is admitted all the same."""
    case, b, A, inv = system
    kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    got = solve_drawn(solver(reg, "hqd_split", case, 1.0, 1.0, defer, props=drawn(static), **kw), b, static, defer)
    assert got[1] == max_iter + 1
    assert_all_same(got, *others(reg, oracle, refs, ("max", precond, max_iter, defer), system, defer, GRID, **kw))


LINE_GRID, LINE_POSITIONS = 40, 704


@pytest.fixture(scope="module", params=[700 * 512, 698 * 512 + 376], ids=["700-chunks", "699-chunks-partial"])
def line(request, oracle):
    return make_system(oracle, synthetic.poisson_block(request.param, 1, 1))


def line_admitted(idle):
    """The gate, then the draw's own check: the drawing workgroups of a queue hold the queue."""
    assert LINE_POSITIONS <= LINE_GRID * GATE_SLOTS
    assert LINE_POSITIONS % XCDS == 0 and (LINE_GRID - idle) % XCDS == 0
    return (LINE_GRID - idle) // XCDS * SLOTS >= LINE_POSITIONS // XCDS


def test_headroom_slots_loaded_by_pigeonhole(reg, oracle, refs, line):
    """A line on the default map: 704 positions, 88 per queue.  With 8 of the 40 workgroups idle, 32 x 22 = 704: the solve is
    complete only if every drawing workgroup fills all 22 slots, the two past the gate's 20 included."""
    assert line_admitted(8) and 4 * SLOTS >= 88
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=18)
    n = line[0].n_cells
    got = solve_drawn(solver(reg, "hqd_line", line[0], 1.0, grid=LINE_GRID, props=FIN0 + drawn(0, 8), **kw), line[1], 0.0)
    assert_all_same(got, *others(reg, oracle, refs, ("line", n), line, 2.0, LINE_GRID, FIN0, **kw))


def test_idle_groups_the_queues_do_not_fit_are_refused(reg, oracle, refs, line):
    """16 idle workgroups leave 3 x 22 < 88 slots per queue: the static map runs, with every workgroup at work."""
    assert not line_admitted(16)
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=18)
    n = line[0].n_cells
    got = solve_drawn(solver(reg, "hqd_refused", line[0], 1.0, grid=LINE_GRID, props=FIN0 + drawn(0, 16), **kw), line[1],
                      float(GATE_SLOTS))
    assert_all_same(got, *others(reg, oracle, refs, ("line", n), line, 2.0, LINE_GRID, FIN0, **kw))


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
def test_most_workgroups_draw_once_and_own_nothing(reg, oracle, refs, precond):
    """30^3 = 53 chunks in 64 positions on the device's full grid, stopped by tolerance: eight positions per queue, so nearly
    every workgroup draws past the end -- some of them after workgroup 0 has passed both waits.  A second solve on the
    handle and one with new coefficients: the heads are cleared and the parity restarts per solve."""
    sysm = make_system(oracle, synthetic.poisson_case(30))
    case, b = sysm[0], sysm[1]
    kw = dict(preconditioner=precond, tolerance=1e-9, rel_tol=0.0, max_iter=300)
    s = solver(reg, "hqd_small", case, 1.0, grid=0, props=FIN0 + drawn(0), **kw)
    first = solve_drawn(s, b, 0.0)
    assert_all_same(first, *others(reg, oracle, refs, ("small", precond), sysm, 2.0, 0, FIN0, **kw))
    assert_same(first, solve_drawn(s, b, 0.0))
    other = synthetic.poisson_case(30)
    rng = np.random.default_rng(20241019)
    other.upper[:] = rng.uniform(-1.0, -0.25, other.upper.size)
    other.diag[:] = rng.uniform(7.0, 9.0, other.n_cells)
    s.set_matrix(other)
    new = solve_drawn(s, b, 0.0)
    assert new[1] != first[1]
    _, _, A2, inv2 = make_system(oracle, other)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A2, b, np.zeros_like(b), inv2 if precond == capi.PRECOND_BJ else None, tolerance=1e-9, rel_tol=0.0,
                        max_iter=300)
    assert ref.n_iterations == new[1]
    np.testing.assert_array_equal(new[2], ref.history)
    np.testing.assert_array_equal(new[0], ref.x)


@pytest.mark.parametrize("graph", [0.0, 1.0])
@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_profiled_turns_between_drawing_launches(reg, oracle, refs, system, defer, graph):
    """profile_kernels 3: every third turn runs k_spmv_sym | k_cg_step2r1x on the static map and touches no head, so the
    parity of the sets must count the held-q launches, not the turns."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=33)
    s = solver(reg, "hqd_mixed", case, 1.0, 1.0, defer, props=drawn(0) + (("hipGraph", graph),), profile_kernels=3, **kw)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("heldQInUse") == 1.0 and s.get_property("heldQStaticSlotsInUse") == 0.0
    assert perf.spmv_launches > 0
    got = (x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals)
    assert_all_same(got, *others(reg, oracle, refs, ("max", capi.PRECOND_BJ, 33, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("graph", [0.0, 1.0])
def test_graph_replay_of_drawing_launches(reg, oracle, refs, system, graph):
    """A batch of 16 launches starts at the same parity every time: the captured batch is replayed, twice per solve."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=60)
    s = solver(reg, "hqd_graph", case, 1.0, props=drawn(0) + (("hipGraph", graph), ("hipGraphCaptures", 0.0)), **kw)
    got = solve_drawn(s, b, 0.0)
    assert_same(got, solve_drawn(s, b, 0.0))
    assert s.get_property("hipGraphCaptures") == (1.0 if graph else 0.0)
    assert_all_same(got, *others(reg, oracle, refs, ("graph",), system, 2.0, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_beta_zero_and_a_stopped_solve_with_drawn_slots(reg, oracle, refs, system, defer):
    """b = 0 from x = 0: beta = 0 in every turn, nothing is updated; and a guess that meets the criterion at the first
    (stand-alone) head: the resident launches that follow return before any draw and leave everything alone."""
    case, b, A, inv = system
    zero = (case, np.zeros_like(b), A, inv)
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=3)
    got = solve_drawn(solver(reg, "hqd_beta0", case, 1.0, 1.0, defer, props=drawn(0), **kw), zero[1], 0.0, defer)
    assert got[1] == 4 and not got[0].any()
    assert_all_same(got, *others(reg, oracle, refs, ("beta0", defer), zero, defer, GRID, **kw))
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=1e-5, rel_tol=0.0, max_iter=600)
    first = solve_drawn(solver(reg, "hqd_tol", case, 1.0, 1.0, defer, props=drawn(0), **kw), b, 0.0, defer)
    assert_all_same(first, *others(reg, oracle, refs, ("tol", defer), system, defer, GRID, **kw))
    kw["tolerance"] = 1e-3  # (well above what the guess leaves)
    s = solver(reg, "hqd_stopped", case, 1.0, 1.0, defer, props=drawn(0), **kw)
    again = solve_drawn(s, b, 0.0, defer, x0=first[0].copy())
    assert again[1] == 1
    np.testing.assert_array_equal(again[0], first[0])
