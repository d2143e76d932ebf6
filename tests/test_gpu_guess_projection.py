"""The initial guess from the last solutions on the device (keyword guessProjection K; kernels_proj.hip, solver_proj.cpp,
DESIGN.md section 7f) against the NumPy walk of the contract (tests/guess_projection_walk.py, pinned by
tests/test_guess_projection_walk.py): (a) the pre-step alone, bit for bit; (b) a solve with the keyword is the same solve
called with the projected guess; (c) a time-step loop; (d) the refusals and what clears the ring.  Every test sets the
keyword through Solver.set_guess_projection, which the parent of this feature does not have."""
import gc

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr
import guess_projection_walk as pw
import soak_worker

pytestmark = pytest.mark.gpu

BOXES = {"6x6x6": (6, 6, 6),        # 216 rows: one chunk
         "10x9x7": (10, 9, 7),      # 630 rows: a partial second chunk
         "9x9x7": (9, 9, 7),        # 567 rows, odd: the one-row tail of the last pair
         "12x12x12": (12, 12, 12)}  # 1,728 rows: four chunks
SYSTEMS = list(BOXES) + ["random"]


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module")
def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


def random_case(n=650, per_row=3, reach=40, seed=20250611):
    """One asymmetric system with irregular faces and a cyclic patch pair, as tests/test_gpu_random_systems.py draws them."""
    rng = np.random.default_rng(seed)
    pairs = set()
    for i in range(n - 1):
        for j in rng.integers(i + 1, min(n, i + 1 + reach), per_row):
            pairs.add((i, int(j)))
    pairs = np.array(sorted(pairs), dtype=np.int32).reshape(-1, 2)
    upper, lower = rng.uniform(-1, 0, len(pairs)), rng.uniform(-1, 0, len(pairs))
    a = rng.choice(n, 6, replace=False).astype(np.int32)
    b = rng.choice(n, 6, replace=False).astype(np.int32)
    ifaces = [synthetic.Interface(synthetic.IFACE_CYCLIC, a, rng.uniform(0, 0.5, 6), -1, 1),
              synthetic.Interface(synthetic.IFACE_CYCLIC, b, rng.uniform(0, 0.5, 6), -1, 0)]
    diag = np.full(n, 1.0)
    np.add.at(diag, pairs[:, 0], np.abs(upper))
    np.add.at(diag, pairs[:, 1], np.abs(lower))
    for itf in ifaces:
        np.add.at(diag, itf.face_cells, np.abs(itf.bou_coeffs))
    return synthetic.LduCase(n, pairs[:, 0].copy(), pairs[:, 1].copy(), diag, upper, lower, ifaces)


_systems = {}


def system(oracle, name):
    """(LduArrays, case, (rp, cols, vals), b, x0, eight ring vectors) of a system, built once and left unchanged."""
    if name not in _systems:
        case = random_case() if name == "random" else synthetic.poisson_block(*BOXES[name])
        rng = np.random.default_rng(len(name) + case.n_cells)
        n = case.n_cells
        _systems[name] = (capi.LduArrays(case), case, oracle_csr(oracle, case), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
                          [rng.uniform(-1, 1, n) for _ in range(8)])
    return _systems[name]


def cfg_of(name, **kw):
    base = dict(solver=capi.SOLVER_BICGSTAB if name == "random" else capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ,
                max_block_size=1, export_res=1, adapt_min_iter=0, update_init_guess=1, matrix_format=capi.FORMAT_CSR,
                tolerance=1e-8, rel_tol=0.0, max_iter=300)
    base.update(kw)
    return capi.default_config(**base)


def pre_step(reg, oracle, chunk_rows, field, name, ring, x0=None, K=8):
    """The device's pre-step alone (maxIter 0: the solve stops at its first check and leaves x as the pre-step made it)
    beside the walk's."""
    arrays, _, (rp, cols, vals), b, x0_default, _ = system(oracle, name)
    x0 = x0_default if x0 is None else x0
    s = reg.solver(field, cfg_of(name, max_iter=0)).set_matrix(arrays)
    s.set_guess_projection(K).set_guess_history(ring)
    x, perf = s.solve(b, x0)
    with blocked(oracle, chunk_rows):
        w = pw.project(oracle, rp, cols, vals, b, x0, ring)
    return s, x, perf, w


def assert_pre_step(s, x, w, k):
    np.testing.assert_array_equal(x, w.x)
    assert s.get_property("guessProjectionOffered") == k == w.offered
    assert s.get_property("guessProjectionKept") == w.kept
    np.testing.assert_array_equal(s.get_property("guessProjectionNormBefore"), w.norm_before)  # (NaN with a NaN in the guess)
    assert s.get_property("guessProjectionLaunches") == k + 5  # 1 + k products, Gram pass, sums, small solve, update


# ---------------------------------------------------------------- (a) the pre-step alone

@pytest.mark.parametrize("k", [1, 4, 5, 8])
@pytest.mark.parametrize("name", SYSTEMS)
def test_pre_step_is_the_walk(reg, oracle, chunk_rows, name, k):
    """k = 1, 4: k_proj_gram<4> and its edge; 5, 8: k_proj_gram<8> and its edge."""
    ring = system(oracle, name)[5][:k]
    s, x, perf, w = pre_step(reg, oracle, chunk_rows, f"gp_pre_{name}", name, ring)
    assert w.kept == k and not np.array_equal(w.x, system(oracle, name)[4])
    assert_pre_step(s, x, w, k)
    # the step of a solve that ran no turn but kept a column: the projected guess minus the caller's
    hist = s.guess_history()
    assert s.get_property("guessProjectionStored") == len(hist) == min(k + 1, 8)
    np.testing.assert_array_equal(hist[-1], w.x - system(oracle, name)[4])
    for got, want in zip(hist[:-1], ring[-7:]):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("kind", ["duplicate", "zero", "nan_column", "one_nan", "nan_in_guess"])
@pytest.mark.parametrize("name", ["10x9x7", "random"])
def test_pre_step_with_dropped_columns(reg, oracle, chunk_rows, name, kind):
    d = system(oracle, name)[5]
    x0 = None
    if kind == "duplicate":
        ring, flags = [d[0], d[1], d[0].copy(), d[2], d[3]], [True, True, False, True, True]
    elif kind == "zero":
        ring, flags = [d[0], np.zeros_like(d[0]), d[1], d[2]], [True, False, True, True]
    elif kind == "nan_column":
        ring, flags = [d[0], np.full_like(d[0], np.nan), d[2]], [True, False, True]
    elif kind == "one_nan":
        bad = d[1].copy()
        bad[17] = np.nan
        ring, flags = [d[0], bad, d[2]], [True, False, True]
    else:  # every alpha is NaN: all of them become +0.0, nothing is kept, the guess stays as it is
        ring, flags = d[:3], [False] * 3
        x0 = system(oracle, name)[4].copy()
        x0[40] = np.nan
    s, x, perf, w = pre_step(reg, oracle, chunk_rows, f"gp_drop_{name}", name, ring, x0)
    assert w.flags == flags
    assert_pre_step(s, x, w, len(ring))
    if kind == "nan_in_guess":
        np.testing.assert_array_equal(x, x0)
        assert s.get_property("guessProjectionStored") == 3  # no column kept, no turn: the slot is abandoned


# ---------------------------------------------------------------- (b) as-if

AS_IF = {
    "GKOCG_none": ("10x9x7", dict(preconditioner=capi.PRECOND_NONE), None),
    "GKOCG_BJ1_half": ("12x12x12", dict(), ("symmetricHalf", 1.0)),
    "GKOCG_BJ1_csr": ("12x12x12", dict(symmetric_half=0, compress_indices=0), ("symmetricHalf", 0.0)),
    "GKOBiCGStab_BJ1": ("random", dict(), None),
    "GKOGMRES10": ("9x9x7", dict(solver=capi.SOLVER_GMRES, krylov_dim=10), None),
    "renumber_on": ("12x12x12", dict(renumber=capi.RENUMBER_ON), None),
    "mixedPrecision": ("10x9x7", dict(), ("mixedPrecisionInUse", 1.0)),
}


@pytest.mark.parametrize("what", list(AS_IF))
def test_a_solve_with_the_keyword_is_the_solve_from_the_projected_guess(reg, oracle, chunk_rows, what):
    name, kw, prop = AS_IF[what]
    arrays, case, _, b, x0, d = system(oracle, name)
    ring = d[:4]
    if what == "renumber_on":
        case = synthetic.renumber_case(case, 300)
        arrays = capi.LduArrays(case)

    def handle(tag, K, **more):
        s = reg.solver(f"gp_asif_{what}_{tag}", cfg_of(name, **kw, **more)).set_matrix(arrays)
        s.set_guess_projection(K)
        if what == "mixedPrecision":
            s.set_mixed_precision(True)
        return s

    guess, _ = handle("pre", 4, max_iter=0).set_guess_history(ring).solve(b, x0)
    assert not np.array_equal(guess, x0)
    with_kw = handle("with", 4).set_guess_history(ring)
    xa, pa = with_kw.solve(b, x0)
    without = handle("without", 0)
    xb, pb = without.solve(b, guess)
    assert with_kw.get_property("guessProjectionKept") == 4
    if what == "renumber_on":
        assert with_kw.renumbering() is not None
    if prop:
        assert with_kw.get_property(prop[0]) == prop[1] == without.get_property(prop[0])
    assert pa.n_iterations > 2
    assert (pa.n_iterations, pa.n_norm_evals) == (pb.n_iterations, pb.n_norm_evals)
    np.testing.assert_array_equal(with_kw.history(), without.history())
    np.testing.assert_array_equal(xa, xb)
    assert (pa.initial_residual, pa.final_residual, pa.norm_factor) == (pb.initial_residual, pb.final_residual, pb.norm_factor)
    # the stored step is the whole one, from the caller's guess
    np.testing.assert_array_equal(with_kw.guess_history()[-1], xa - x0)


# ---------------------------------------------------------------- (c) a time-step loop

@pytest.fixture(scope="module")
def walked(oracle, chunk_rows):
    with blocked(oracle, chunk_rows):
        return {K: pw.run_sequence(oracle, K, 10, lambda c: oracle_csr(oracle, c)) for K in (0, 4)}


def test_time_step_loop(oracle, walked):
    """The sequence of tests/test_guess_projection_walk.py on the device, the handle fetched anew every step as a time-step
    loop does: every step is the walk's bit for bit, the iterations of steps 4 .. 9 fall below half, the ledger stands still
    from the second step on and nothing is left after close."""
    gc.collect()
    base = capi.memory_ledger().as_dict()
    r = capi.Registry()
    its, marks = {0: [], 4: []}, []
    try:
        for K in (4, 0):
            x = np.zeros(np.prod(pw.SEQ_SHAPE))
            for n in range(10):
                case = pw.sequence_case(n)
                b = pw.sequence_rhs(case, n)
                s = r.solver(f"gp_seq_{K}", cfg_of("10x9x7", max_iter=1000, **pw.SEQ_CRITERION)).set_matrix(case)
                s.set_guess_projection(K)
                x, perf = s.solve(b, x)
                p, res, ring = walked[K][n]
                msg = f"K = {K}, step {n}"
                assert perf.n_iterations == res.n_iterations, msg
                np.testing.assert_array_equal(s.history(), res.history, err_msg=msg)
                np.testing.assert_array_equal(x, res.x, err_msg=msg)
                if K:
                    assert (s.get_property("guessProjectionOffered"), s.get_property("guessProjectionKept"),
                            s.get_property("guessProjectionStored")) == (p.offered, p.kept, len(ring)), msg
                    assert s.get_property("guessProjectionNormBefore") == p.norm_before, msg
                    hist = s.guess_history()
                    assert len(hist) == len(ring), msg
                    for got, want in zip(hist, ring):
                        np.testing.assert_array_equal(got, want, err_msg=msg)
                    marks.append(capi.memory_ledger().as_dict())
                its[K].append(perf.n_iterations)
        print("K = 0:", its[0], "\nK = 4:", its[4])
        assert sum(its[4][4:]) < 0.5 * sum(its[0][4:])
        for later in marks[2:]:
            for key in soak_worker.LEDGER_EXACT + ("device_alloc_calls", "pinned_alloc_calls"):
                assert later[key] == marks[1][key], (key, marks)
    finally:
        r.close()
    after = capi.memory_ledger().as_dict()
    for key in soak_worker.LEDGER_EXACT:
        assert after[key] == base[key], (key, after, base)
    assert after["unknown_frees"] == 0


# ---------------------------------------------------------------- (d) refusals and clearing

def test_refusals(reg, oracle):
    arrays, _, _, b, x0, d = system(oracle, "10x9x7")
    s = reg.solver("gp_bad", cfg_of("10x9x7", max_iter=5)).set_matrix(arrays)
    for bad in (9, 2.5, -1):
        s.set_guess_projection(bad)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, x0)
        assert e.value.status == capi.ERR_INVALID and "guessProjection" in str(e.value)
    s.set_guess_projection(2)
    with pytest.raises(capi.OglError) as e:
        s.set_guess_history(d[:3])
    assert e.value.status == capi.ERR_INVALID
    s.set_guess_history(d[:2]).solve(b, x0)  # the handle goes on after a refusal
    assert s.get_property("guessProjectionOffered") == 2 and s.get_property("guessProjectionStored") == 2


def test_two_ranks_are_refused(oracle):
    """A host communicator of size 2 in one process: the solve fails before anything of it is enqueued (the callbacks are
    never reached by it), and the message names the rank count."""
    arrays, _, _, b, x0, _ = system(oracle, "6x6x6")
    r2 = capi.Registry()
    try:
        r2.set_host_comm(0, 2, lambda v: v, lambda nbr, cnt, send: send)
        s = r2.solver("gp_two", cfg_of("6x6x6", max_iter=3)).set_matrix(arrays)
        s.set_guess_projection(4)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, x0)
        assert e.value.status == capi.ERR_UNSUPPORTED
        assert "guessProjection" in str(e.value) and "2 ranks" in str(e.value)
    finally:
        r2.close()


def test_what_clears_the_ring(reg, oracle):
    arrays, _, _, b, x0, d = system(oracle, "10x9x7")
    other = system(oracle, "9x9x7")

    def filled(field):
        s = reg.solver(field, cfg_of("10x9x7", max_iter=5)).set_matrix(arrays)
        s.set_guess_projection(4).set_guess_history(d[:2])
        s.solve(b, x0)
        assert len(s.guess_history()) == 3
        return s

    s = filled("gp_clear_pattern")
    s.set_matrix(arrays)  # new coefficients on the same pattern keep it
    assert len(s.guess_history()) == 3
    s.set_matrix(other[0])  # a pattern change
    assert s.guess_history().shape == (0, other[1].n_cells)
    s.solve(other[3], other[4])
    assert s.get_property("guessProjectionOffered") == 0 and s.get_property("guessProjectionStored") == 1

    s = filled("gp_clear_k")
    s.set_guess_projection(3)  # a change of K
    assert len(s.guess_history()) == 0
    s.solve(b, x0)
    assert s.get_property("guessProjectionOffered") == 0 and s.get_property("guessProjectionStored") == 1

    s = filled("gp_clear_reset")
    s.set_property("guessProjectionReset", 1.0)
    assert len(s.guess_history()) == 0 and s.get_property("guessProjectionReset") == 0.0
    s.set_guess_history(d[:1])
    s.set_property("guessProjectionReset", 1.0)
    s.solve(b, x0)  # ... taken up by the next solve as well
    assert s.get_property("guessProjectionOffered") == 0 and s.get_property("guessProjectionStored") == 1
    s.set_guess_history([])
    assert len(s.guess_history()) == 0


def test_k0_after_k4_is_the_plain_solve(reg, oracle):
    arrays, _, _, b, x0, d = system(oracle, "10x9x7")
    plain = reg.solver("gp_plain", cfg_of("10x9x7")).set_matrix(arrays)
    plain.set_guess_projection(0)
    xp, pp = plain.solve(b, x0)
    s = reg.solver("gp_back", cfg_of("10x9x7")).set_matrix(arrays)
    s.set_guess_projection(4).set_guess_history(d[:4])
    x4, p4 = s.solve(b, x0)
    assert s.get_property("guessProjectionKept") == 4 and not np.array_equal(s.history(), plain.history())
    s.set_guess_projection(0)
    x0_again, p0 = s.solve(b, x0)
    assert (p0.n_iterations, p0.n_norm_evals) == (pp.n_iterations, pp.n_norm_evals)
    np.testing.assert_array_equal(s.history(), plain.history())
    np.testing.assert_array_equal(x0_again, xp)
    assert len(s.guess_history()) == 0
