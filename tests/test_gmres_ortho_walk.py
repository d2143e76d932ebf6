"""The NumPy walk of the GKOGMRES loop with a selectable Gram-Schmidt step (tests/gmres_ortho_walk.py)
on its own, on the CPU: with "mgs" it is the committed oracle bit for bit, which pins the walk; "cgs" and "cgs2" give other
bits than "mgs" from the second column on, so the GPU tests (tests/test_gpu_gmres_ortho.py) cannot pass on a solve that
stayed on modified Gram-Schmidt; and a "cgs2" solve to the default criterion meets it on the true residual."""
import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import blocked, oracle_csr
from mixed_walk import meets_criterion
import gmres_ortho_walk as gw

CHUNK_ROWS = 512  # the device's reduction chunk (ogl_reduction_chunk_rows)
SHAPE = (13, 9, 11)  # 1,287 rows: three chunks, the last partial

_systems = {}


def system(oracle, sym):
    if sym not in _systems:
        kw = {} if sym else dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
        case = synthetic.poisson_block(*SHAPE, **kw)
        b = synthetic.rhs_for_x_star(case)[0]
        _systems[sym] = (oracle_csr(oracle, case), b)
    return _systems[sym]


def walk(oracle, sym, bj, ortho, **kw):
    (rp, cols, vals), b = system(oracle, sym)
    P = oracle.Precond(rp, cols, vals, 1) if bj else None
    with blocked(oracle, CHUNK_ROWS):
        return gw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), P, ortho, **kw)


@pytest.mark.parametrize("krylov_dim,max_iter", [(1, 3), (4, 8), (4, 10), (10, 10), (10, 17)])
@pytest.mark.parametrize("bj", [False, True], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_mgs_walk_is_the_oracle(oracle, sym, bj, krylov_dim, max_iter):
    """maxIter at a restart, at the end of a cycle and inside one ((4, 10), (10, 17)); the residual export on."""
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=max_iter, krylov_dim=krylov_dim)
    w = walk(oracle, sym, bj, "mgs", **kw)
    (rp, cols, vals), b = system(oracle, sym)
    P = oracle.Precond(rp, cols, vals, 1) if bj else None
    with blocked(oracle, CHUNK_ROWS):
        ref = oracle.gmres(oracle.DistMatrix(rp, cols, vals), b, np.zeros_like(b), P, **kw)
    assert (w.n_iterations, w.n_evals) == (ref.n_iterations, ref.n_evals) == (max_iter + 1, max_iter + 1)
    np.testing.assert_array_equal(w.history, ref.history)
    np.testing.assert_array_equal(w.x, ref.x)
    assert (w.initial_residual, w.final_residual, w.norm_factor) == (ref.initial_residual, ref.final_residual, ref.norm_factor)


@pytest.mark.parametrize("bj", [False, True], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_mgs_walk_is_the_oracle_to_a_tolerance(oracle, sym, bj):
    """A stop by the criterion (which sees a new residual only after a restart), with minIter in play (checks 1 .. 6 pass
    without a verdict)."""
    kw = dict(tolerance=1e-4, rel_tol=0.0, max_iter=200, min_iter=7, krylov_dim=10)
    w = walk(oracle, sym, bj, "mgs", **kw)
    (rp, cols, vals), b = system(oracle, sym)
    P = oracle.Precond(rp, cols, vals, 1) if bj else None
    with blocked(oracle, CHUNK_ROWS):
        ref = oracle.gmres(oracle.DistMatrix(rp, cols, vals), b, np.zeros_like(b), P, **kw)
    assert (w.n_iterations, w.n_evals) == (ref.n_iterations, ref.n_evals) and w.n_iterations < 200
    np.testing.assert_array_equal(w.history, ref.history)
    np.testing.assert_array_equal(w.x, ref.x)


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("bj", [False, True], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_block_forms_are_not_mgs(oracle, sym, bj, ortho):
    """Column 0 has one basis vector and one dot product on the untouched w: cgs is mgs there (cgs2 adds its second
    coefficient already).  From column 1 on the dot products of cgs see another w than those of mgs: other bits in H --
    not in every column, a difference below the rounding of a sum leaves a column alone -- hence in x."""
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=10, krylov_dim=10)
    ref, w = walk(oracle, sym, bj, "mgs", **kw), walk(oracle, sym, bj, ortho, **kw)
    assert [it for it, _ in w.columns] == [it for it, _ in ref.columns] == list(range(10))
    if ortho == "cgs":
        assert w.columns[0] == ref.columns[0]
    differing = [it for (it, col), (_, col_ref) in zip(w.columns, ref.columns) if it >= 1 and col != col_ref]
    print(f"{ortho}: columns that differ from mgs {differing}, max |x - x_mgs| {np.abs(w.x - ref.x).max():.3e}")
    assert len(differing) >= 5
    assert not np.array_equal(w.x, ref.x)
    # the same Krylov space in exact arithmetic: x agrees far beyond what a wrong formula would leave
    np.testing.assert_allclose(w.x, ref.x, rtol=0, atol=1e-9 * np.abs(ref.x).max())


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_cgs2_meets_the_default_criterion_on_the_true_residual(oracle, sym):
    (rp, cols, vals), b = system(oracle, sym)
    kw = dict(tolerance=1e-6, rel_tol=1e-6)
    w = walk(oracle, sym, True, "cgs2", max_iter=1000, krylov_dim=30, **kw)
    assert w.n_iterations < 1000 and meets_criterion(w.final_residual, w.initial_residual, **kw)
    true = gw.true_residual(oracle, rp, cols, vals, b, w.x, w.norm_factor)
    print(f"cgs2: {w.n_iterations} checks, recorded {w.final_residual:.3e}, true {true:.3e}")
    assert meets_criterion(true, w.initial_residual, **kw)
