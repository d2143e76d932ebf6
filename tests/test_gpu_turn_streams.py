"""The cache policy of the resident CG turn's streams (resident_cg_turn.hpp; DESIGN.md section 4.3, "Streams of the resident
turn").  A load or store that goes past the caches computes what the plain one computes, so the policy shows nowhere but
where the code around it has two paths or two kernels: the 16-byte pair against the scalar tail of a partial pair (the
system's last row), and r handed between k_cg_turn_held_q and the pair k_spmv_sym | k_cg_step2r1x, which run the same body.
Exactly that is pinned here; everything else about the turn is in test_gpu_held_z*.py and test_gpu_held_q*.py.

Every case is compared bit for bit -- residual history, x, iteration count, final residual, norm evaluations -- with the
same solve by the three-launch turn (heldZ 0), whose kernels keep the plain policy.  The helpers are those of
test_gpu_held_q.py; a reference is computed once per configuration and shared."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from test_gpu_held_q import assert_same, solve, solver

pytestmark = pytest.mark.gpu
CHUNK = 512
GRID = 32   # heldZGrid: 640 chunks on 32 workgroups are 20 each -- 11 (13 where phase S draws) in registers, the rest in LDS
FIN0 = (("fusedFinMaxChunks", 0.0),)  # (below 1,025 chunks every workgroup would reduce for itself: no leader turn)
# 640 chunks, the last of one row (a partial pair: the scalar path), and of two rows (one full pair, then nothing)
LINES = {"one-row-chunk": 640 * CHUNK - 511, "one-pair-chunk": 640 * CHUNK - 510}
# name -> (heldQ, properties): the two-launch turn, the one-launch turn on the static map (slots 0 .. 10 registers, 11 .. 19
# LDS, the last chunk in LDS slot 8 of workgroup 31) and as it runs by default, with the positions behind slot 12 drawn
SHAPES = {
    "two-launch": (0.0, ()),
    "one-launch-static": (1.0, (("heldQStaticSlots", 20.0),)),
    "one-launch-drawn": (1.0, ()),
}
BJ, NONE = capi.PRECOND_BJ, capi.PRECOND_NONE


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _cases.clear()
    _refs.clear()


_cases = {}
_refs = {}


def system(key, make):
    if key not in _cases:
        case = make()
        _cases[key] = (case, synthetic.rhs_for_x_star(case)[0])
    return _cases[key]


def line(which):
    return system(which, lambda: synthetic.poisson_block(LINES[which], 1, 1))


def test_geometry():
    """The arithmetic the cases rest on."""
    for rows, last in ((LINES["one-row-chunk"], 1), (LINES["one-pair-chunk"], 2)):
        assert -(-rows // CHUNK) == 640 == GRID * 20 and rows - 639 * CHUNK == last
    assert 31 % 2 == 1 and (31 * 31 * 79) % 2 == 1   # (the box below: an odd line length, an odd row count)
    assert 4 * GRID < -(-31 * 31 * 79 // CHUNK) <= 5 * GRID   # (every workgroup owns four or five chunks)


def three_launch(reg, key, case, b, defer, props=FIN0, x0=None, **kw):
    """The same solve with heldZ 0, once per key."""
    if key not in _refs:
        _refs[key] = solve(solver(reg, "ts_ref", case, 0.0, 0.0, defer, GRID, props, **kw), b, 0.0, 0.0, defer, x0)
    return _refs[key]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("precond", [BJ, NONE], ids=["BJ", "none"])
@pytest.mark.parametrize("which", list(LINES))
def test_pair_path_meets_scalar_tail(reg, which, precond, defer, shape):
    """Fully loaded workgroups whose last slot ends in a partial pair or in a single full one; stops at both ring
    positions."""
    case, b = line(which)
    held_q, props = SHAPES[shape]
    for max_iter in (17, 18):
        kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
        got = solve(solver(reg, "ts_line", case, held_q, 1.0, defer, GRID, FIN0 + props, **kw), b, held_q, 1.0, defer)
        assert got[1] == max_iter + 1
        assert_same(got, three_launch(reg, (which, precond, defer, max_iter), case, b, defer, **kw))


@pytest.mark.parametrize("shape", ["one-launch-static", "one-launch-drawn"])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("which", list(LINES))
def test_the_two_kernel_shapes_hand_r_to_each_other(reg, which, defer, shape):
    """profile_kernels 2: every second turn runs k_spmv_sym | k_cg_step2r1x, the others k_cg_turn_held_q, and each reads the r
    (and p, and the pending x term) that the other has stored."""
    case, b = line(which)
    held_q, props = SHAPES[shape]
    kw = dict(preconditioner=BJ, tolerance=0.0, rel_tol=0.0, max_iter=18)
    s = solver(reg, "ts_mixed", case, held_q, 1.0, defer, GRID, FIN0 + props, profile_kernels=2, **kw)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("heldQInUse") == 1.0 and s.get_property("heldZInUse") == 1.0
    assert perf.spmv_launches > 0
    got = (x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals)
    assert_same(got, three_launch(reg, (which, BJ, defer, 18), case, b, defer, **kw))


def record_lows(h, after):
    """The first odd and the first even turn past `after` whose residual is below every earlier one."""
    lows = [k for k in range(after + 1, len(h)) if h[k] < h[:k].min()]
    return next(k for k in lows if k % 2 == 1), next(k for k in lows if k % 2 == 0)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_second_solve_stops_by_tolerance_at_either_parity(reg, defer, shape):
    """A second solve on the handle, from the first one's x, stopped by a tolerance that lies between a record low of the
    three-launch turn's own history and the lowest value before it: once at an odd turn, once at an even one.  With
    deferX 2 one of the two stops on a deferring head, which puts its own term of x in at the stop, from its one
    (non-temporal) read of p; the other on a head that updates x, which reads p_pend for the term pending before it, as
    every second head of a deferX 2 solve does."""
    case, b = line("one-row-chunk")
    held_q, props = SHAPES[shape]
    first_kw = dict(preconditioner=BJ, tolerance=0.0, rel_tol=0.0, max_iter=18)
    first = three_launch(reg, ("one-row-chunk", BJ, defer, 18), case, b, defer, **first_kw)
    probe = three_launch(reg, ("second-probe", defer), case, b, defer, x0=first[0].copy(),
                         preconditioner=BJ, tolerance=0.0, rel_tol=0.0, max_iter=120)
    h = probe[2]
    for turn in record_lows(h, 6):
        tol = float(np.sqrt(h[turn] * h[:turn].min()))
        assert h[turn] < tol < h[:turn].min()
        kw = dict(preconditioner=BJ, tolerance=tol, rel_tol=0.0, max_iter=600)
        ref = three_launch(reg, ("second", defer, turn), case, b, defer, x0=first[0].copy(), **kw)
        assert ref[1] == turn + 1
        s = solver(reg, "ts_second", case, held_q, 1.0, defer, GRID, FIN0 + props, **kw)
        # (the first solve under the second one's criterion: it only has to leave the handle used; max_iter is the
        # configuration's, so it is stopped by the same tolerance, far later or not at all within 600 turns)
        warm = solve(s, b, held_q, 1.0, defer)
        assert warm[1] > 1
        got = solve(s, b, held_q, 1.0, defer, x0=first[0].copy())
        assert got[1] == turn + 1
        assert_same(got, ref)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("precond", [BJ, NONE], ids=["BJ", "none"])
def test_odd_box_runs_the_rolled_early_x_loop(reg, precond, defer, shape):
    """31 x 31 x 79: the line length is odd, so the pair-load (FAST) instantiations are off, and the row count is odd, so
    the last pair is partial.  149 chunks on 32 workgroups: four or five slots each, the first heldZEarlySlots = 4 of them
    written by the rolled early-x loop of a head that updates x, the fifth by the last loop."""
    case, b = system("box31", lambda: synthetic.poisson_block(31, 31, 79))
    held_q, props = SHAPES[shape]
    props = FIN0 + props + (("heldZEarlySlots", 4.0),)
    for max_iter in (17, 18):
        kw = dict(preconditioner=precond, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
        got = solve(solver(reg, "ts_box", case, held_q, 1.0, defer, GRID, props, **kw), b, held_q, 1.0, defer)
        assert got[1] == max_iter + 1
        assert_same(got, three_launch(reg, ("box31", precond, defer, max_iter), case, b, defer, **kw))
