"""The NumPy walk of the mixed-precision contract (tests/mixed_walk.py) on its own, on the CPU: the
conditions on the inputs that the GPU tests (tests/test_gpu_mixed_precision.py) rely on -- how many outer steps the boxes
take, that they end by the criterion, that no fp32 intermediate is subnormal (subnormal behaviour is deliberately not
pinned), and that the answer meets the criterion on the true fp64 residual."""
import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import blocked, oracle_csr
import mixed_walk as mw

CHUNK_ROWS = 512  # the device's reduction chunk (ogl_reduction_chunk_rows)
BOXES = {"10x9x7": (10, 9, 7),   # 630 rows: two chunks, the second partial
         "6x6x6": (6, 6, 6)}     # one partial chunk


def system(oracle, shape):
    case = synthetic.poisson_block(*shape)
    b = synthetic.rhs_for_x_star(case)[0]
    rp, cols, vals = oracle_csr(oracle, case)
    return case, rp, cols, vals, b


def walk(oracle, shape, jacobi, **kw):
    case, rp, cols, vals, b = system(oracle, shape)
    inv_d = oracle.jacobi_generate_scalar(rp, cols, vals) if jacobi else None
    with blocked(oracle, CHUNK_ROWS):
        w = mw.mixed_walk(oracle, rp, cols, vals, b, np.zeros_like(b), inv_d, **kw)
    return w, (rp, cols, vals, b)


@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "BJ1"])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_tight_tolerance_needs_refinement(oracle, box, jacobi):
    kw = dict(tolerance=1e-10, rel_tol=0.0)
    w, (rp, cols, vals, b) = walk(oracle, BOXES[box], jacobi, **kw)
    assert w.outer_steps >= 2 and w.stop_reason == mw.STOP_CRITERION
    assert w.n_evals == w.outer_steps + 1 == w.history.size and w.n_iterations == w.inner_turns + 1
    assert w.smallest_fp32 >= mw.TINY32
    assert np.all(np.diff(w.history) < 0)
    true = mw.true_residual(oracle, rp, cols, vals, b, w.x, w.norm_factor)
    assert mw.meets_criterion(true, w.initial_residual, **kw)


@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "BJ1"])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_loose_tolerance_is_one_outer_step(oracle, box, jacobi):
    kw = dict(tolerance=1e-10, rel_tol=0.01)
    w, (rp, cols, vals, b) = walk(oracle, BOXES[box], jacobi, **kw)
    assert w.outer_steps == 1 and w.stop_reason == mw.STOP_CRITERION
    assert w.smallest_fp32 >= mw.TINY32
    true = mw.true_residual(oracle, rp, cols, vals, b, w.x, w.norm_factor)
    assert mw.meets_criterion(true, w.initial_residual, **kw)


def test_budgets_and_edges(oracle):
    """The other walks the GPU tests use: where each ends and why."""
    shape = BOXES["10x9x7"]
    tight = dict(tolerance=1e-10, rel_tol=0.0)
    full, (rp, cols, vals, b) = walk(oracle, shape, True, **tight)
    # innerMaxIter 5: every inner solve ends by its budget
    w, _ = walk(oracle, shape, True, inner_max_iter=5, **tight)
    # (restarted every five turns, sum |r| does not fall monotonically: the walk ends on "no progress", honestly)
    assert w.outer_steps > 2 and all(t == 5 for t in w.step_turns)
    assert w.stop_reason in (mw.STOP_CRITERION, mw.STOP_NO_PROGRESS)
    assert w.smallest_fp32 >= mw.TINY32
    # maxIter inside the second inner solve
    t1 = full.step_turns[0]
    w, _ = walk(oracle, shape, True, max_iter=t1 + 3, **tight)
    assert w.outer_steps == 2 and w.inner_turns == t1 + 3 and w.stop_reason == mw.STOP_MAX_ITER
    assert w.smallest_fp32 >= mw.TINY32
    # minIter above the first outer step's turns: its check is not evaluated
    loose = dict(tolerance=1e-10, rel_tol=0.01)
    t1 = walk(oracle, shape, True, **loose)[0].step_turns[0]
    w, _ = walk(oracle, shape, True, min_iter=t1 + 1, **loose)
    assert w.outer_steps == 2 and w.n_evals == 2 and w.stop_reason == mw.STOP_CRITERION and w.step_turns == [t1, 1]
    assert w.smallest_fp32 >= mw.TINY32
    assert full.inner_turns > t1 + 3 and full.step_turns[1] > 3

