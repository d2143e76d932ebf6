"""The contract of the keyword guessProjection on the CPU: tests/guess_projection_walk.py against
numpy.linalg.lstsq, its dropping rule, the order of the ring, and the time-step sequence the GPU test runs on the device
(tests/test_gpu_guess_projection.py) -- the projection has to halve the oracle's CG iterations there."""
import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import blocked, oracle_csr
import guess_projection_walk as pw

CHUNK_ROWS = 512


def box(oracle, shape, seed=0):
    case = synthetic.poisson_block(*shape)
    rng = np.random.default_rng(seed)
    n = case.n_cells
    return oracle_csr(oracle, case), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng


@pytest.fixture(scope="module")
def sequences(oracle):
    """The ten steps with K = 0 and K = 4, computed once."""
    with blocked(oracle, CHUNK_ROWS):
        return {K: pw.run_sequence(oracle, K, 10, lambda c: oracle_csr(oracle, c)) for K in (0, 4)}


def test_k0_and_an_empty_ring_leave_the_guess_untouched(oracle):
    (rp, cols, vals), b, x0, rng = box(oracle, (10, 9, 7))
    with blocked(oracle, CHUNK_ROWS):
        p = pw.project(oracle, rp, cols, vals, b, x0, [])
        assert p.kept == 0 and p.offered == 0
        np.testing.assert_array_equal(p.x, x0)
        ring = pw.Ring(0)
        ring.store(x0)
        assert ring.vectors == []
        A = oracle.DistMatrix(rp, cols, vals)
        plain = oracle.cg(A, b, x0, None, tolerance=0.0, rel_tol=0.0, max_iter=5)
        p, res = pw.step(oracle, ring, rp, cols, vals, b, x0,
                         lambda g: oracle.cg(A, b, g, None, tolerance=0.0, rel_tol=0.0, max_iter=5), lambda r: True)
        np.testing.assert_array_equal(res.x, plain.x)
        np.testing.assert_array_equal(res.history, plain.history)
        assert ring.vectors == [] and p.stored == 0


# relative distance of |r0 - W alpha|_2 from numpy.linalg.lstsq's on the kept columns.  Measured on this walk: at most
# 1.6e-16 over the random rings below (0 in 11 of 12 cases) and 3.6e-10 over the rings of the sequence (whose vectors are
# nearly dependent and whose r0 lies almost inside their span, so the norm left over is small against r0).  The bounds are
# two orders of magnitude over these.
LSTSQ_BOUND_RANDOM = 2e-14    # measured 1.6e-16
LSTSQ_BOUND_SEQUENCE = 4e-8   # measured 3.6e-10


def lstsq_gap(p):
    keep = [j for j, f in enumerate(p.flags) if f]
    W = np.array(p.W).T
    mine = np.linalg.norm(p.r0 - W @ np.array(p.alpha))
    ref = np.linalg.norm(p.r0 - W[:, keep] @ np.linalg.lstsq(W[:, keep], p.r0, rcond=None)[0])
    return abs(mine - ref) / ref


@pytest.mark.parametrize("k", [1, 4, 5, 8])
@pytest.mark.parametrize("shape", [(6, 6, 6), (10, 9, 7), (12, 12, 12)], ids=str)
def test_residual_is_the_least_squares_one(oracle, shape, k):
    (rp, cols, vals), b, x0, rng = box(oracle, shape, seed=1)
    ring = [rng.uniform(-1, 1, b.size) for _ in range(k)]
    with blocked(oracle, CHUNK_ROWS):
        p = pw.project(oracle, rp, cols, vals, b, x0, ring)
    assert p.kept == k
    gap = lstsq_gap(p)
    print(f"{shape} k = {k}: relative gap to lstsq {gap:.2e}")
    assert gap <= LSTSQ_BOUND_RANDOM
    # the projection can only lower the residual's 2-norm
    r1 = oracle.spmv_adv(rp, cols, vals, -1.0, p.x, 1.0, b)
    assert np.linalg.norm(r1) < np.linalg.norm(p.r0)


def test_residual_is_the_least_squares_one_on_the_sequence(sequences):
    gaps = [lstsq_gap(p) for p, _, _ in sequences[4] if p.kept]
    print("relative gap to lstsq per step:", " ".join(f"{g:.2e}" for g in gaps))
    assert len(gaps) == 9 and max(gaps) <= LSTSQ_BOUND_SEQUENCE


def test_dropped_columns(oracle):
    (rp, cols, vals), b, x0, rng = box(oracle, (10, 9, 7), seed=2)
    n = b.size
    d = [rng.uniform(-1, 1, n) for _ in range(3)]
    with blocked(oracle, CHUNK_ROWS):
        clean = pw.project(oracle, rp, cols, vals, b, x0, d)
        dup = pw.project(oracle, rp, cols, vals, b, x0, [d[0], d[1], d[0].copy(), d[2]])
        zero = pw.project(oracle, rp, cols, vals, b, x0, [d[0], np.zeros(n), d[1], d[2]])
        bad = d[1].copy()
        bad[:] = np.nan
        nan = pw.project(oracle, rp, cols, vals, b, x0, [d[0], bad, d[2]])
        one_nan = d[1].copy()
        one_nan[17] = np.nan
        nan1 = pw.project(oracle, rp, cols, vals, b, x0, [d[0], one_nan, d[2]])
    assert clean.kept == 3 and clean.flags == [True] * 3
    # an exact duplicate: its pivot is 0 up to rounding, far below 2^-32 of G_jj; the others see the clean problem
    assert dup.flags == [True, True, False, True] and dup.alpha[2] == 0.0 and not np.signbit(dup.alpha[2])
    np.testing.assert_array_equal([dup.alpha[0], dup.alpha[1], dup.alpha[3]], clean.alpha)
    np.testing.assert_array_equal(dup.x, clean.x)
    # a zero vector: G_jj = 0 and 0 > 0 fails
    assert zero.flags == [True, False, True, True] and zero.alpha[1] == 0.0
    np.testing.assert_array_equal([zero.alpha[0], zero.alpha[2], zero.alpha[3]], clean.alpha)
    np.testing.assert_array_equal(zero.x, clean.x)
    # a column of NaN, or with one NaN: G_jj is NaN and fails the comparison.  The sums of step 5 run over kept columns
    # only, so the NaN of G_ij reaches no other column: the column is dropped alone and the others see the clean problem
    # of two.  The update still walks the column (0 x NaN), so x carries its NaN where the column has one.
    with blocked(oracle, CHUNK_ROWS):
        two = pw.project(oracle, rp, cols, vals, b, x0, [d[0], d[2]])
    for p in (nan, nan1):
        assert p.flags == [True, False, True] and p.alpha[1] == 0.0 and not np.signbit(p.alpha[1])
        np.testing.assert_array_equal([p.alpha[0], p.alpha[2]], two.alpha)
    assert np.isnan(nan.x).all()
    assert np.isnan(nan1.x[17])
    np.testing.assert_array_equal(np.delete(nan1.x, 17), np.delete(two.x, 17))
    # the non-finite case: a NaN in the guess makes r0, hence g and every alpha, NaN -- every alpha becomes +0.0, nothing
    # counts as kept and the guess comes back as it was
    x_bad = x0.copy()
    x_bad[40] = np.nan
    with blocked(oracle, CHUNK_ROWS):
        p = pw.project(oracle, rp, cols, vals, b, x_bad, d)
    assert p.kept == 0 and p.alpha == [0.0, 0.0, 0.0] and not any(np.signbit(p.alpha))
    np.testing.assert_array_equal(p.x, x_bad)


def test_ring_order_after_k_plus_two_stores():
    K = 4
    ring = pw.Ring(K)
    for i in range(K + 2):
        ring.store(np.full(3, float(i)))
        assert len(ring.vectors) == min(i + 1, K)
    assert [v[0] for v in ring.vectors] == [2.0, 3.0, 4.0, 5.0]  # oldest first, the two oldest gone


def test_sequence_halves_the_iterations(sequences):
    """10 x 9 x 7, coefficients varied per step, x*(t) in four fixed modes, dt 0.1, tolerance 1e-9, relTol 0, the oracle's
    Jacobi-CG from each projected guess: the iterations of steps 4 .. 9."""
    its = {K: [res.n_iterations for _, res, _ in sequences[K]] for K in (0, 4)}
    kept = [p.kept for p, _, _ in sequences[4]]
    print("K = 0:", its[0], "\nK = 4:", its[4], "kept", kept)
    assert sum(its[4][4:]) < 0.5 * sum(its[0][4:])
    assert [p.offered for p, _, _ in sequences[4]] == [0, 1, 2, 3, 4, 4, 4, 4, 4, 4]
    assert [len(r) for _, _, r in sequences[4]] == [1, 2, 3, 4, 4, 4, 4, 4, 4, 4]
    assert its[0][:1] == its[4][:1]  # step 0 has nothing to project on
    for _, res, _ in sequences[4]:
        assert res.final_residual <= 1e-9
