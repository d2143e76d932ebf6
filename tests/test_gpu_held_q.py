"""The held-q turn of single-rank GKOCG on half storage (kernels_spmv_sym.hip, k_cg_turn_held_q): the SpMV, beta, step_2r,
the check, the pending x update and step_1 of the next turn in ONE resident kernel that keeps q = A p and then z = r / d in
registers and LDS -- one launch per turn instead of the held-z turn's two.  The row sums are k_spmv_sym's, the partials keep
their tree, the three sums the finaliser's order: history, x, iteration count, final residual and the number of norm
evaluations carry the bits of the two-launch turn (heldQ 0), of the three-launch turn (heldZ 0) and of the oracle in the
device's reduction order, wherever the criterion stops.

The default gate switches the turn on where the half storage streams; the sizes here are far below that, so every test
forces it with the property and asserts heldQInUse.  heldZGrid lowers the number of resident workgroups, so that a small
system loads every slot of a workgroup: 11 in registers, 9 in LDS.  A workgroup's slots are POSITIONS of the SpMV's launch
order (the band order with its holes, or the padded default map), not chunks."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_matrix

pytestmark = pytest.mark.gpu
N = 84      # 592,704 rows = 1,158 chunks in a band order of 1,176 positions (with holes)
GRID = 59   # 55 workgroups own 20 positions, 4 own 19: every register slot, every LDS slot, the prefetch of the last two


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
    """What the other turns and the oracle give, computed once per configuration."""
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
    assert s.get_property("symmetricHalf") == 1.0 and s.get_property("symmetricHalfPerChunk") == 0.0
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
        two = solve(solver(reg, "hq_ref2", case, 0.0, 1.0, defer, grid, props, **kw), b, 0.0, 1.0, defer, x0)
        three = solve(solver(reg, "hq_ref3", case, 0.0, 0.0, defer, grid, props, **kw), b, 0.0, 0.0, defer, x0)
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


@pytest.mark.parametrize("early", [1.0, 0.0])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("max_iter", [1, 2, 16, 17, 33])
def test_same_bits_wherever_max_iter_stops(reg, oracle, refs, system, precond, max_iter, defer, early):
    """Stops in every batch of 16 turns and at both ring positions, with x updated before the sums or behind them."""
    case, b, A, inv = system
    kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    got = solve(solver(reg, "hq_max", case, 1.0, 1.0, defer, props=(("heldZEarlyX", early),), **kw), b, 1.0, 1.0, defer)
    assert got[1] == max_iter + 1
    assert_all_same(got, *others(reg, oracle, refs, ("max", precond, max_iter, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("tol", [1e-2, 1e-5])
def test_stop_by_tolerance_and_frequency(reg, oracle, refs, system, tol, defer):
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=tol, rel_tol=0.0, max_iter=600, eval_frequency=3)
    got = solve(solver(reg, "hq_tol", case, 1.0, 1.0, defer, **kw), b, 1.0, 1.0, defer)
    assert got[1] % 3 == 1 and got[4] == (got[1] + 2) // 3  # (checks 0, 3, 6, ... are the evaluated ones)
    assert_all_same(got, *others(reg, oracle, refs, ("tol", tol, defer), system, defer, GRID, **kw))


@pytest.fixture(scope="module")
def long_history(oracle, system):
    """The oracle's residuals of 200 turns (the L1 norm rises before it falls): where the cases below place their stops."""
    case, b, A, inv = system
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        return oracle.cg(A, b, np.zeros_like(b), inv, tolerance=0.0, rel_tol=0.0, max_iter=200).history


def record_low(h, after):
    """The first turn past `after` whose residual is below every earlier one."""
    return next(k for k in range(after + 1, len(h)) if h[k] < h[:k].min())


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("after", [4, 40])
def test_stop_by_rel_tol_at_a_stated_turn(reg, oracle, refs, system, long_history, after, defer):
    """rel_tol between two entries of the oracle's own history: the check of the first record low past turn `after` is
    the first that meets it, in the first batch of turns and in a later one."""
    case, b, A, inv = system
    h = long_history
    turn = record_low(h, after)
    rel = float(np.sqrt(h[turn] * h[:turn].min())) / h[0]
    assert h[turn] < rel * h[0] < h[:turn].min()
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=rel, max_iter=600)
    got = solve(solver(reg, "hq_rel", case, 1.0, 1.0, defer, **kw), b, 1.0, 1.0, defer)
    assert got[1] == turn + 1
    assert_all_same(got, *others(reg, oracle, refs, ("rel", after, defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_stop_by_min_iter_at_a_stated_turn(reg, oracle, refs, system, long_history, defer):
    """A tolerance that the check of turn M (the first record low) would meet, and minIter M + 3: the checks 1 .. M + 2 give
    no verdict, the one of turn M + 3 is the second that is evaluated and stops."""
    case, b, A, inv = system
    h = long_history
    first = record_low(h, 0)
    stop = first + 3
    tol = float(np.sqrt(max(h[first], h[stop]) * h[0]))
    assert h[first] < tol and h[stop] < tol <= h[0]
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=tol, rel_tol=0.0, max_iter=600, min_iter=stop)
    got = solve(solver(reg, "hq_min", case, 1.0, 1.0, defer, **kw), b, 1.0, 1.0, defer)
    assert got[1] == stop + 1 and got[4] == 2
    assert_all_same(got, *others(reg, oracle, refs, ("min", defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_odd_line_length(reg, oracle, refs, defer):
    """83^3: the rows of a lane are no aligned pair of the strips, the instantiation without pair loads."""
    sysm = make_system(oracle, synthetic.poisson_case(83))
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=20)
    got = solve(solver(reg, "hq_odd", sysm[0], 1.0, 1.0, defer, grid=64, **kw), sysm[1], 1.0, 1.0, defer)
    assert_all_same(got, *others(reg, oracle, refs, ("odd", defer), sysm, defer, 64, **kw))


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("box", [(640, 512, 1), (639, 512, 1), (327680, 1, 1), (327068, 1, 1)],
                         ids=["2d-640", "2d-639-odd", "1d-640", "1d-639-partial"])
def test_two_and_one_dimensions_on_the_default_map(reg, oracle, refs, box, precond):
    """Three and two planes, no band order: the positions are the default map's, 640 of them for 640 and for 639 chunks --
    exactly what 32 workgroups hold, every slot loaded (the 639-chunk systems leave one position without a chunk)."""
    sysm = make_system(oracle, synthetic.poisson_block(*box))
    kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=18)
    props = (("fusedFinMaxChunks", 0.0),)  # (below 1,025 chunks every workgroup would reduce for itself: no leader turn)
    got = solve(solver(reg, "hq_dim", sysm[0], 1.0, grid=32, props=props, **kw), sysm[1], 1.0)
    assert_all_same(got, *others(reg, oracle, refs, ("dim", box, precond), sysm, 2.0, 32, props, **kw))


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE])
@pytest.mark.parametrize("grid", [0, 32])
def test_partial_last_chunk(reg, oracle, refs, precond, grid):
    """30^3 = 27,000 rows = 53 chunks in 64 positions, the last chunk of 376 rows (fusedFinMaxChunks 0 puts the leader turn
    on from 48 chunks).  grid 0: the device's full resident grid, most of whose workgroups own nothing."""
    sysm = make_system(oracle, synthetic.poisson_case(30))
    kw = dict(preconditioner=precond, tolerance=1e-9, rel_tol=0.0, max_iter=300)
    props = (("fusedFinMaxChunks", 0.0),)
    got = solve(solver(reg, "hq_part", sysm[0], 1.0, grid=grid, props=props, **kw), sysm[1], 1.0)
    assert_all_same(got, *others(reg, oracle, refs, ("part", precond, grid), sysm, 2.0, grid, props, **kw))


def test_positions_decide_the_capacity(reg, oracle, refs, system):
    """58 workgroups hold 1,160 slots: the 1,158 chunks fit, the 1,176 positions do not -- the two-launch turn runs although
    the one-launch turn is asked for, with the same bits.  (Exactly full: the 640 positions on 32 workgroups above.)"""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=17)
    two = solve(solver(reg, "hq_cap", case, 1.0, grid=58, **kw), b, 0.0, 1.0)
    assert_same(two, others(reg, oracle, refs, ("max", capi.PRECOND_BJ, 17, 2.0), system, 2.0, GRID, **kw)[0])


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_profiled_turns_run_the_two_launch_turn(reg, oracle, refs, system, defer):
    """profile_kernels 3: every third turn carries an event pair and runs the stand-alone SpMV and the held-z kernel, the
    others the one-launch kernel; both leave the same state behind."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=33)
    s = solver(reg, "hq_mixed", case, 1.0, 1.0, defer, profile_kernels=3, **kw)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("heldQInUse") == 1.0 and perf.spmv_launches > 0
    got = (x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals)
    assert_all_same(got, *others(reg, oracle, refs, ("max", capi.PRECOND_BJ, 33, defer), system, defer, GRID, **kw))


def test_a_second_solve_a_converged_guess_and_new_coefficients(reg, oracle, system):
    """The tagged box is cleared and the tags restart with every solve; a guess that already satisfies the criterion stops at
    the first (stand-alone) head and the resident kernels that follow leave everything alone; new coefficients on the same
    pattern reach the planes the kernel reads."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=1e-8, rel_tol=0.0, max_iter=600)
    s, off = solver(reg, "hq_twice", case, 1.0, **kw), solver(reg, "hq_twice_off", case, 0.0, **kw)
    first = solve(s, b, 1.0)
    assert_same(first, solve(s, b, 1.0))
    assert_same(first, solve(off, b, 0.0))
    third = solve(s, b, 1.0, x0=first[0].copy())
    assert third[1] == 1
    np.testing.assert_array_equal(third[0], first[0])
    other = synthetic.poisson_case(N)
    rng = np.random.default_rng(20241016)
    other.upper[:] = rng.uniform(-1.0, -0.25, other.upper.size)
    other.diag[:] = rng.uniform(7.0, 9.0, other.n_cells)
    s.set_matrix(other)
    off.set_matrix(other)
    fourth = solve(s, b, 1.0)
    assert fourth[1] != first[1]
    assert_same(fourth, solve(off, b, 0.0))
    _, _, A2, inv2 = make_system(oracle, other)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A2, b, np.zeros_like(b), inv2, tolerance=1e-8, rel_tol=0.0, max_iter=600)
    assert ref.n_iterations == fourth[1]
    np.testing.assert_array_equal(fourth[2], ref.history)
    np.testing.assert_array_equal(fourth[0], ref.x)


@pytest.mark.parametrize("graph", [0.0, 1.0])
@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_graph_replay_on_and_off(reg, oracle, refs, system, graph, defer):
    """Batches of 16 turns replayed from one captured graph (the first batch, with the stand-alone head, runs direct)."""
    case, b, A, inv = system
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=60)
    s = solver(reg, "hq_graph", case, 1.0, 1.0, defer, props=(("hipGraph", graph), ("hipGraphCaptures", 0.0)), **kw)
    got = solve(s, b, 1.0, 1.0, defer)
    assert (s.get_property("hipGraphCaptures") >= 1.0) == (graph == 1.0)
    again = solve(s, b, 1.0, 1.0, defer)  # (the second solve replays what the first has captured)
    assert s.get_property("hipGraphCaptures") == (1.0 if graph else 0.0)
    assert_same(got, again)
    assert_all_same(got, *others(reg, oracle, refs, ("graph", defer), system, defer, GRID, **kw))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_beta_zero(reg, oracle, refs, system, defer):
    """b = 0 from x = 0: r = p = q = 0 and beta = p.q = 0 in every turn -- no update of r or x, the turns run to maxIter."""
    case, b, A, inv = system
    zero = (case, np.zeros_like(b), A, inv)
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=3)
    got = solve(solver(reg, "hq_beta0", case, 1.0, 1.0, defer, **kw), zero[1], 1.0, 1.0, defer)
    assert got[1] == 4 and not got[0].any()
    assert_all_same(got, *others(reg, oracle, refs, ("beta0", defer), zero, defer, GRID, **kw))


@pytest.mark.parametrize("chunks", [2048, 2049, 4097])
def test_the_three_tagged_sums_at_the_virtual_thread_edges(reg, oracle, refs, chunks):
    """One partial more than two per virtual thread of the finaliser's order, and one more than four: 1-D systems on the
    device's full resident grid, beta, rho and sum |r'| each summed from tagged words."""
    sysm = make_system(oracle, synthetic.poisson_block((chunks - 1) * 512 + 1, 1, 1))
    kw = dict(preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0, max_iter=4)
    got = solve(solver(reg, "hq_sums", sysm[0], 1.0, grid=0, **kw), sysm[1], 1.0)
    assert_all_same(got, *others(reg, oracle, refs, ("sums", chunks), sysm, 2.0, 0, **kw))
