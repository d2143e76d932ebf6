"""The NumPy walk of the GKOGMRES loop with a selectable precision of the stored basis (tests/gmres_basis_walk.py,
DESIGN.md section 7e) on its own, on the CPU: with basis "double" it is tests/gmres_ortho_walk.gmres_walk bit for bit, which
pins it; with "single" every stored vector is a binary32 vector, the bits leave those of the double basis as soon as the
criterion sees a residual that was formed through a stored vector, no store lands in the unpinned range below 2^-126 on
any system of tests/test_gpu_gmres_basis.py, and the solve to a tolerance stays inside the cap that test fixes."""
import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import blocked, oracle_csr
from mixed_walk import meets_criterion
import gmres_ortho_walk as gw
import gmres_basis_walk as bw

CHUNK_ROWS = 512  # the device's reduction chunk (ogl_reduction_chunk_rows)
# the boxes of tests/test_gpu_gmres_basis.py that a CPU test can walk in a few seconds, and its line of 513 rows
SHAPES = {"7x7x7": (7, 7, 7), "13x9x11": (13, 9, 11), "513x1x1": (513, 1, 1)}
TOL = dict(tolerance=1e-6, rel_tol=0.0, krylov_dim=30)  # the stop by tolerance of the GPU file

_systems = {}


def system(oracle, shape, sym):
    if (shape, sym) not in _systems:
        kw = {} if sym else dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
        case = synthetic.poisson_block(*SHAPES[shape], **kw)
        b = synthetic.rhs_for_x_star(case)[0]
        _systems[shape, sym] = (oracle_csr(oracle, case), b)
    return _systems[shape, sym]


def walks(oracle, shape, sym, block, ortho, basis, **kw):
    """(gmres_ortho_walk's walk or None, gmres_basis_walk's)."""
    (rp, cols, vals), b = system(oracle, shape, sym)
    P = oracle.Precond(rp, cols, vals, block) if block else None
    with blocked(oracle, CHUNK_ROWS):
        ref = gw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), P, ortho, **kw) if basis == "double" else None
        return ref, bw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), P, ortho, basis, **kw)


def assert_same_walk(w, ref):
    assert (w.n_iterations, w.n_evals) == (ref.n_iterations, ref.n_evals)
    np.testing.assert_array_equal(w.history, ref.history)
    np.testing.assert_array_equal(w.x, ref.x)
    assert w.columns == ref.columns
    assert (w.initial_residual, w.final_residual, w.norm_factor) == (ref.initial_residual, ref.final_residual, ref.norm_factor)


@pytest.mark.parametrize("ortho", ["mgs", "cgs", "cgs2"])
@pytest.mark.parametrize("bj", [0, 1], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_double_basis_is_the_ortho_walk(oracle, sym, bj, ortho):
    """Two full cycles and a partial third, in the device's tree."""
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=12, krylov_dim=5)
    ref, w = walks(oracle, "13x9x11", sym, bj, ortho, "double", **kw)
    assert_same_walk(w, ref)
    assert w.subnormal_stores == 0 and all(v.dtype == np.float64 for v in w.basis)


@pytest.mark.parametrize("ortho", ["mgs", "cgs", "cgs2"])
@pytest.mark.parametrize("bj", [0, 1], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_double_basis_is_the_ortho_walk_with_numpy_sums(oracle, sym, bj, ortho):
    """The same outside helpers.blocked (the oracle's own order of summation), to a tolerance."""
    (rp, cols, vals), b = system(oracle, "13x9x11", sym)
    P = oracle.Precond(rp, cols, vals, 1) if bj else None
    kw = dict(tolerance=1e-4, rel_tol=0.0, max_iter=200, min_iter=7, krylov_dim=10)
    ref = gw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), P, ortho, **kw)
    w = bw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), P, ortho, "double", **kw)
    assert w.n_iterations < 200
    assert_same_walk(w, ref)


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("bj", [0, 1], ids=["none", "BJ1"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_single_basis_stores_binary32_and_leaves_the_double_bits(oracle, sym, bj, ortho):
    """The criterion sees sum|r| of the last restart, and the restart follows the check of the turn that filled the cycle:
    the checks 0 .. krylovDim repeat the residual of x0, formed before anything was stored, and are equal; from check
    krylovDim + 1 on -- the second residual evaluated -- every x came through rounded basis vectors and the bits differ."""
    for m, first_new in ((1, 2), (5, 6)):
        kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=12, krylov_dim=m)
        _, d = walks(oracle, "13x9x11", sym, bj, ortho, "double", **kw)
        _, s = walks(oracle, "13x9x11", sym, bj, ortho, "single", **kw)
        assert s.n_iterations == d.n_iterations == 13
        assert s.norm_factor == d.norm_factor
        np.testing.assert_array_equal(s.history[:first_new], d.history[:first_new])
        assert np.all(s.history[first_new:] != d.history[first_new:]), (m, s.history, d.history)
        assert not np.array_equal(s.x, d.x)
        for v in s.basis:
            assert v.dtype == np.float32 and v.shape == d.x.shape
            np.testing.assert_array_equal(v.astype(np.float64).astype(np.float32), v)
            assert np.abs(v).max() <= 1.0
        # every operation runs in double on nearly the same vectors: x agrees to the rounding of the basis, 2^-24 per entry
        np.testing.assert_allclose(s.x, d.x, rtol=0, atol=1e-5 * np.abs(d.x).max())


@pytest.mark.parametrize("block", [0, 1, 4], ids=["none", "BJ1", "BJ4"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_store_below_the_normal_range(oracle, shape, sym, block):
    """What the bit-exact GPU tests run on these systems (12 turns, krylovDim 30 holds the most vectors; 13x9x11 also a
    cycle of 40): a store in (0, 2^-126) is not pinned, so there must be none."""
    for ortho in ("cgs", "cgs2"):
        _, w = walks(oracle, shape, sym, block, ortho, "single", tolerance=0.0, rel_tol=0.0, max_iter=12, krylov_dim=30)
        assert w.subnormal_stores == 0
    if shape == "13x9x11" and not sym and block == 1:
        _, w = walks(oracle, shape, sym, block, "cgs2", "single", tolerance=0.0, rel_tol=0.0, max_iter=40, krylov_dim=40)
        assert w.subnormal_stores == 0 and len(w.basis) == 41


def tolerance_cap(oracle, ortho):
    """maxIter of the GPU file's stop by tolerance: twice the turns of the DOUBLE walk (a condition fixed before the single
    walk runs, not a measurement of it)."""
    _, d = walks(oracle, "13x9x11", False, 1, ortho, "double", max_iter=1000, **TOL)
    assert d.n_iterations < 1000
    return 2 * (d.n_iterations - 1), d


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
def test_single_basis_stops_by_tolerance_inside_twice_the_double_turns(oracle, ortho):
    cap, d = tolerance_cap(oracle, ortho)
    _, s = walks(oracle, "13x9x11", False, 1, ortho, "single", max_iter=cap, **TOL)
    (rp, cols, vals), b = system(oracle, "13x9x11", False)
    true = gw.true_residual(oracle, rp, cols, vals, b, s.x, s.norm_factor)
    print(f"{ortho}: double {d.n_iterations - 1} turns, single {s.n_iterations - 1} (cap {cap}); recorded "
          f"{s.final_residual:.3e}, true {true:.3e}")
    assert s.n_iterations - 1 < cap  # (the check that stops at maxIter is check number cap)
    assert meets_criterion(s.final_residual, s.initial_residual, tolerance=1e-6, rel_tol=0.0)
    assert meets_criterion(true, s.initial_residual, tolerance=1e-6, rel_tol=0.0)
    assert s.subnormal_stores == 0
