"""The keyword guessProjectionCredit on the device (k_proj_credit in kernels_proj.hip, criterion_verdict in
device_common.hpp, solver_proj.cpp).  With the credit the criterion's initial residual is
S0 / norm_factor, S0 = sum |b - A x0| at the caller's guess, and nothing else of the solve changes -- so the credited solve
with (tolerance T, relTol R) has to be, bit for bit, the K = 0 solve from the projected guess with tolerance
max(T, R * init_res) and relTol 0: (1) that equivalence for every solver and layout; (2) a projection that already meets
the criterion ends the solve at its first check; (3) nothing to credit: the plain solve; (4) a time-step loop against the
walk (tests/guess_projection_credit_walk.py) with the keyword switched between steps; (5) refusals; (6) the keyword
guessProjectionProducts onePass (k_proj_products_sym in kernels_spmv_sym.hip): the bits of the separate products, and of the
walk's.  Systems, rings' sizes and cfg_of are those of tests/test_gpu_guess_projection.py; what the oracle says about these inputs is held by
tests/test_guess_projection_credit_walk.py."""
import gc

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr
import guess_projection_walk as pw
import guess_projection_credit_walk as cw
import test_gpu_guess_projection as base

pytestmark = pytest.mark.gpu

T, R = cw.SINGLE_TOLERANCE, cw.SINGLE_REL_TOL


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module")
def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


CONFIGS = {
    "GKOCG_none": (dict(preconditioner=capi.PRECOND_NONE), None),
    "GKOCG_BJ1_half": (dict(), ("symmetricHalf", 1.0)),
    "GKOCG_BJ1_csr": (dict(symmetric_half=0, compress_indices=0), ("symmetricHalf", 0.0)),
    "GKOBiCGStab_BJ1": (dict(), None),
    "GKOGMRES10": (dict(solver=capi.SOLVER_GMRES, krylov_dim=10), None),
    "renumber_on": (dict(renumber=capi.RENUMBER_ON), None),
}


def threshold(S0, norm_factor, tolerance, rel_tol):
    """(init_res, the tolerance of the equivalent K = 0 solve): one IEEE division, one rounded product."""
    init_res = float(np.float64(S0) / np.float64(norm_factor))
    return init_res, max(tolerance, float(np.float64(rel_tol) * np.float64(init_res)))


def assert_same_solve(sa, xa, pa, sb, xb, pb, initial=True):
    assert (pa.n_iterations, pa.n_norm_evals) == (pb.n_iterations, pb.n_norm_evals)
    np.testing.assert_array_equal(sa.history(), sb.history())
    np.testing.assert_array_equal(xa, xb)
    assert (pa.final_residual, pa.norm_factor) == (pb.final_residual, pb.norm_factor)
    if initial:
        assert pa.initial_residual == pb.initial_residual


# ---------------------------------------------------------------- (1) the equivalence

@pytest.mark.parametrize("what", list(CONFIGS))
def test_credited_solve_is_the_k0_solve_with_the_credited_threshold(reg, oracle, what):
    name = cw.SINGLE[what][0]
    kw, prop = CONFIGS[what]
    arrays, case, csr, b, x0, _ = base.system(oracle, name)
    ring = cw.single_ring(what, csr, b, x0)
    if what == "renumber_on":
        case = synthetic.renumber_case(case, 300)
        arrays = capi.LduArrays(case)

    def handle(tag, K, **more):
        s = reg.solver(f"gpc_eq_{what}_{tag}", base.cfg_of(name, **kw, **more)).set_matrix(arrays)
        return s.set_guess_projection(K)

    guess, _ = handle("pre", 4, max_iter=0).set_guess_history(ring).solve(b, x0)
    assert not np.array_equal(guess, x0)
    built = handle("built", 4, rel_tol=R).set_guess_history(ring)
    _, p_built = built.solve(b, x0)
    credited = handle("credited", 4, rel_tol=R).set_guess_projection_credit(1).set_guess_history(ring)
    xa, pa = credited.solve(b, x0)
    assert credited.get_property("guessProjectionCreditInUse") == 1.0
    assert credited.get_property("guessProjectionKept") == 4
    S0 = credited.get_property("guessProjectionNormBefore")
    assert S0 == built.get_property("guessProjectionNormBefore") and built.get_property("guessProjectionCreditInUse") == 0.0
    init_res, thr = threshold(S0, pa.norm_factor, T, R)
    assert pa.initial_residual == init_res
    assert p_built.initial_residual < init_res and p_built.norm_factor == pa.norm_factor  # as built: counted from the projected guess
    plain = handle("plain", 0, tolerance=thr, rel_tol=0.0)
    xb, pb = plain.solve(b, guess)
    print(f"{what}: checks as built {p_built.n_iterations}, credited {pa.n_iterations}; init_res {init_res:.3e} "
          f"against {p_built.initial_residual:.3e}")
    assert_same_solve(credited, xa, pa, plain, xb, pb, initial=False)
    assert pa.n_iterations <= p_built.n_iterations - 2  # (the oracle's counts: tests/test_guess_projection_credit_walk.py)
    if what == "renumber_on":
        assert credited.renumbering() is not None
    if prop:
        assert credited.get_property(prop[0]) == prop[1] == plain.get_property(prop[0])
    # the stored step is the whole one, from the caller's guess
    np.testing.assert_array_equal(credited.guess_history()[-1], xa - x0)


# ---------------------------------------------------------------- (2) the stop at the first check

@pytest.mark.parametrize("what", cw.FIRST_CHECK)
def test_a_projection_that_meets_the_criterion_ends_the_solve_at_its_first_check(reg, oracle, what):
    """tolerance 0, so that relTol alone decides (guess_projection_credit_walk.FIRST_CHECK): the projected guess is x* up
    to rounding, which any tolerance would accept with or without the credit."""
    name = cw.SINGLE[what][0]
    kw, _ = CONFIGS[what]
    arrays, _, csr, b, x0, _ = base.system(oracle, name)
    ring = [cw.x_star_of(*csr, b) - x0]

    def handle(tag, **more):
        cfg = base.cfg_of(name, **kw, tolerance=cw.FIRST_CHECK_TOLERANCE, **more)
        s = reg.solver(f"gpc_first_{what}_{tag}", cfg).set_matrix(arrays)
        return s.set_guess_projection(4).set_guess_history(ring)

    guess, _ = handle("pre", max_iter=0).solve(b, x0)
    s = handle("credited", rel_tol=R).set_guess_projection_credit(1)
    x, perf = s.solve(b, x0)
    assert s.get_property("guessProjectionCreditInUse") == 1.0 and s.get_property("guessProjectionKept") == 1
    # GKOBiCGStab counts whole turns (ogl_perf::n_iterations = checks / 2): one check is 0 turns
    assert perf.n_norm_evals == 1 and perf.n_iterations == (0 if what == "GKOBiCGStab_BJ1" else 1)
    assert len(s.history()) == 1 and perf.final_residual == s.history()[0]
    assert perf.final_residual < R * perf.initial_residual
    assert perf.initial_residual == s.get_property("guessProjectionNormBefore") / perf.norm_factor
    np.testing.assert_array_equal(x, guess)
    hist = s.guess_history()
    assert len(hist) == 2
    np.testing.assert_array_equal(hist[-1], guess - x0)
    # without the credit the same solve goes on: its relTol is counted from the projected guess
    _, p_built = handle("built", rel_tol=R, max_iter=cw.FIRST_CHECK_BUILT_MAX_ITER).solve(b, x0)
    print(f"{what}: as built {p_built.n_iterations} counted, {p_built.n_norm_evals} norms; initial "
          f"{p_built.initial_residual:.3e} against the credited {perf.initial_residual:.3e}")
    assert p_built.n_iterations > perf.n_iterations
    assert p_built.initial_residual == perf.final_residual  # (the credited solve's one check is the built one's first)


# ---------------------------------------------------------------- (3) nothing to credit

def test_an_empty_ring_is_the_plain_solve(reg, oracle):
    arrays, _, _, b, x0, _ = base.system(oracle, "10x9x7")
    plain = reg.solver("gpc_empty_plain", base.cfg_of("10x9x7", rel_tol=R)).set_matrix(arrays)
    xp, pp = plain.solve(b, x0)
    s = reg.solver("gpc_empty", base.cfg_of("10x9x7", rel_tol=R)).set_matrix(arrays)
    s.set_guess_projection(4).set_guess_projection_credit(1)
    x, perf = s.solve(b, x0)
    assert s.get_property("guessProjectionOffered") == 0 and s.get_property("guessProjectionCreditInUse") == 0.0
    assert_same_solve(s, x, perf, plain, xp, pp)
    # credit 1 with K = 0 is the plain solve as well
    s0 = reg.solver("gpc_k0", base.cfg_of("10x9x7", rel_tol=R)).set_matrix(arrays)
    s0.set_guess_projection(0).set_guess_projection_credit(1)
    x, perf = s0.solve(b, x0)
    assert_same_solve(s0, x, perf, plain, xp, pp)


@pytest.mark.parametrize("name", ["10x9x7", "random"])
def test_with_every_column_dropped_the_solve_is_the_one_from_the_callers_guess(reg, oracle, name):
    arrays, _, _, b, x0, _ = base.system(oracle, name)
    plain = reg.solver(f"gpc_drop_plain_{name}", base.cfg_of(name, rel_tol=R)).set_matrix(arrays)
    xp, pp = plain.solve(b, x0)
    s = reg.solver(f"gpc_drop_{name}", base.cfg_of(name, rel_tol=R)).set_matrix(arrays)
    s.set_guess_projection(4).set_guess_projection_credit(1).set_guess_history([np.zeros_like(b)] * 3)
    x, perf = s.solve(b, x0)
    assert s.get_property("guessProjectionOffered") == 3 and s.get_property("guessProjectionKept") == 0
    assert s.get_property("guessProjectionCreditInUse") == 0.0
    assert_same_solve(s, x, perf, plain, xp, pp)
    # (the sum the credit would have used is the solve's own first norm, the same bits)
    assert s.get_property("guessProjectionNormBefore") / perf.norm_factor == perf.initial_residual


# ---------------------------------------------------------------- (4) a time-step loop

CREDIT_OFF_AT = (4, 7)  # the keyword switched off for these steps and on again, on one handle


@pytest.fixture(scope="module")
def walked(oracle, chunk_rows):
    with blocked(oracle, chunk_rows):
        return cw.run_sequence(oracle, 4, 10, lambda c: oracle_csr(oracle, c), 0.05, lambda n: n not in CREDIT_OFF_AT)


def test_time_step_loop(oracle, walked):
    """The sequence of tests/test_guess_projection_credit_walk.py at relTol 0.05 on the device: every step is the walk's bit
    for bit, and the ledger stands still from the third step on."""
    gc.collect()
    r = capi.Registry()
    its, marks = [], []
    try:
        x = np.zeros(np.prod(pw.SEQ_SHAPE))
        for n in range(10):
            case = pw.sequence_case(n)
            b = pw.sequence_rhs(case, n)
            cfg = base.cfg_of("10x9x7", max_iter=1000, tolerance=cw.SEQ_TOLERANCE, rel_tol=0.05)
            s = r.solver("gpc_seq", cfg).set_matrix(case)
            s.set_guess_projection(4).set_guess_projection_credit(0 if n in CREDIT_OFF_AT else 1)
            x, perf = s.solve(b, x)
            p, res, ring, credited = walked[n]
            msg = f"step {n}"
            assert perf.n_iterations == res.n_iterations, msg
            np.testing.assert_array_equal(s.history(), res.history, err_msg=msg)
            np.testing.assert_array_equal(x, res.x, err_msg=msg)
            assert perf.initial_residual == res.initial_residual, msg
            assert (s.get_property("guessProjectionOffered"), s.get_property("guessProjectionKept"),
                    s.get_property("guessProjectionStored")) == (p.offered, p.kept, len(ring)), msg
            assert s.get_property("guessProjectionCreditInUse") == float(credited), msg
            hist = s.guess_history()
            assert len(hist) == len(ring), msg
            for got, want in zip(hist, ring):
                np.testing.assert_array_equal(got, want, err_msg=msg)
            marks.append(capi.memory_ledger().as_dict())
            its.append(perf.n_iterations)
        print("checks per step:", its)
        assert [c for *_, c in walked] == [n >= 1 and n not in CREDIT_OFF_AT for n in range(10)]
        assert 1 in its  # a step that ends at its first check
        for later in marks[3:]:
            assert later["device_alloc_calls"] == marks[2]["device_alloc_calls"], marks
    finally:
        r.close()


# ---------------------------------------------------------------- (5) refusals

def test_refusals(reg, oracle):
    arrays, _, _, b, x0, d = base.system(oracle, "10x9x7")
    s = reg.solver("gpc_bad", base.cfg_of("10x9x7", max_iter=5, rel_tol=R)).set_matrix(arrays)
    s.set_guess_projection(4).set_guess_history(d[:2])
    for bad in (2, 0.5, -1):
        s.set_guess_projection_credit(bad)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, x0)
        assert e.value.status == capi.ERR_INVALID and "guessProjectionCredit" in str(e.value)
    s.set_guess_projection_credit(1).set_mixed_precision(True)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, x0)
    assert e.value.status == capi.ERR_UNSUPPORTED
    assert "guessProjectionCredit" in str(e.value) and "mixedPrecision" in str(e.value)
    s.set_mixed_precision(False)
    s.solve(b, x0)  # the handle goes on after a refusal, the ring as it was
    assert s.get_property("guessProjectionOffered") == 2 and s.get_property("guessProjectionCreditInUse") == 1.0


# ---------------------------------------------------------------- (6) the products in one pass of the matrix

ONE_PASS_BOXES = {"127x1x1": (127, 1, 1),    # ND 2
                  "9x7x1": (9, 7, 1),        # ND 3, an odd line length: not FAST
                  "10x9x7": (10, 9, 7),      # FAST, a partial second chunk
                  "9x9x7": (9, 9, 7),        # not FAST, the one-row tail of the last pair
                  "12x12x12": (12, 12, 12)}  # FAST, four chunks
_one_pass = {}


def one_pass_system(oracle, name):
    """(LduArrays, csr, b, x0, eight ring vectors): base.system's where it has the box, built alike where not."""
    if name in base.BOXES:
        arrays, _, csr, b, x0, d = base.system(oracle, name)
        return arrays, csr, b, x0, d
    if name not in _one_pass:
        case = synthetic.poisson_block(*ONE_PASS_BOXES[name])
        rng = np.random.default_rng(len(name) + case.n_cells)
        n = case.n_cells
        _one_pass[name] = (capi.LduArrays(case), oracle_csr(oracle, case), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
                           [rng.uniform(-1, 1, n) for _ in range(8)])
    return _one_pass[name]


def products_run(reg, field, arrays, cfg, products, stream, ring, b, x0, K=8):
    s = reg.solver(field, cfg).set_matrix(arrays)
    s.set_property("streamAboveBytes", stream)
    s.set_guess_projection(K).set_guess_projection_products(products).set_guess_history(ring)
    x, perf = s.solve(b, x0)
    return s, x, perf


@pytest.mark.parametrize("stream", [0.0, 1e18], ids=["stream", "cached"])
@pytest.mark.parametrize("k", [1, 4, 5, 8])
@pytest.mark.parametrize("name", list(ONE_PASS_BOXES))
def test_one_pass_products_have_the_bits_of_the_separate_ones(reg, oracle, chunk_rows, name, k, stream):
    """maxIter 0: x is what the pre-step made of it.  One pass against the k + 1 products and against the walk."""
    arrays, (rp, cols, vals), b, x0, d = one_pass_system(oracle, name)
    ring = d[:k]
    cfg = base.cfg_of("10x9x7", max_iter=0)
    one, x1, _ = products_run(reg, f"gpp_one_{name}", arrays, cfg, "onePass", stream, ring, b, x0)
    sep, x2, _ = products_run(reg, f"gpp_sep_{name}", arrays, cfg, "separate", stream, ring, b, x0)
    with blocked(oracle, chunk_rows):
        w = pw.project(oracle, rp, cols, vals, b, x0, ring)
    assert one.get_property("symmetricHalf") == 1.0 == sep.get_property("symmetricHalf")
    assert one.get_property("guessProjectionOnePassInUse") == 1.0 and sep.get_property("guessProjectionOnePassInUse") == 0.0
    assert one.get_property("guessProjectionLaunches") == 5 and sep.get_property("guessProjectionLaunches") == k + 5
    assert w.kept == k and not np.array_equal(w.x, x0)
    for s, x in ((one, x1), (sep, x2)):
        np.testing.assert_array_equal(x, w.x)
        assert s.get_property("guessProjectionKept") == w.kept
        assert s.get_property("guessProjectionNormBefore") == w.norm_before
    for got, other in zip(one.guess_history(), sep.guess_history()):
        np.testing.assert_array_equal(got, other)
    np.testing.assert_array_equal(one.guess_history()[-1], w.x - x0)


@pytest.mark.parametrize("stream", [0.0, 1e18], ids=["stream", "cached"])
@pytest.mark.parametrize("name", ["10x9x7", "9x9x7"])
def test_one_pass_products_on_a_ring_that_has_wrapped(reg, oracle, chunk_rows, name, stream):
    """K = 4 after six solves: the stored vectors are two runs of slots.  Every solve is the separate run's, the last
    pre-step the walk's on the ring read back before it."""
    arrays, (rp, cols, vals), b, x0, d = one_pass_system(oracle, name)
    runs = {}
    for products in ("onePass", "separate"):
        s = reg.solver(f"gpp_wrap_{products}_{name}_{stream}", base.cfg_of("10x9x7", max_iter=3)).set_matrix(arrays)
        s.set_property("streamAboveBytes", stream)
        s.set_guess_projection(4).set_guess_projection_products(products).set_guess_history([])
        out = []
        for i in range(7):
            rhs = b + 0.1 * i * d[i]
            before = s.guess_history()
            x, perf = s.solve(rhs, x0)
            out.append((x, s.history(), s.get_property("guessProjectionLaunches"), s.get_property("guessProjectionKept"),
                        s.get_property("guessProjectionNormBefore"), before, rhs))
        runs[products] = (s, out)
    for i, (a, c) in enumerate(zip(runs["onePass"][1], runs["separate"][1])):
        np.testing.assert_array_equal(a[0], c[0], err_msg=f"solve {i}")
        np.testing.assert_array_equal(a[1], c[1], err_msg=f"solve {i}")
        assert a[3:5] == c[3:5], i
        k = min(i, 4)
        # (the ring is full after four stores and turns with the fifth: from solve 5 on the vectors are two runs of slots)
        if k:
            assert (a[2], c[2]) == (5 + (1 if i >= 5 else 0), k + 5 + (1 if i >= 5 else 0)), i
    assert runs["onePass"][0].get_property("guessProjectionOnePassInUse") == 1.0
    # the last pre-step against the walk on the ring as it stood
    x, hist, launches, kept, s0, before, rhs = runs["onePass"][1][6]
    assert launches == 6 and len(before) == 4
    with blocked(oracle, chunk_rows):
        w = pw.project(oracle, rp, cols, vals, rhs, x0, list(before))
    assert (kept, s0) == (w.kept, w.norm_before)


def test_one_pass_keyword_on_the_device_csr_runs_the_separate_products(reg, oracle, chunk_rows):
    arrays, (rp, cols, vals), b, x0, d = one_pass_system(oracle, "12x12x12")
    cfg = base.cfg_of("12x12x12", max_iter=0, symmetric_half=0, compress_indices=0)
    s, x, _ = products_run(reg, "gpp_csr", arrays, cfg, "onePass", 1e18, d[:4], b, x0)
    with blocked(oracle, chunk_rows):
        w = pw.project(oracle, rp, cols, vals, b, x0, d[:4])
    assert s.get_property("symmetricHalf") == 0.0 and s.get_property("guessProjectionOnePassInUse") == 0.0
    assert s.get_property("guessProjectionLaunches") == 4 + 5
    np.testing.assert_array_equal(x, w.x)
    assert s.get_property("guessProjectionNormBefore") == w.norm_before
    s.set_property("guessProjectionProducts", 2.0)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, x0)
    assert e.value.status == capi.ERR_INVALID and "guessProjectionProducts" in str(e.value)
