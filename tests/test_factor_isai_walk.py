"""What the walk of the keywords triangularSolves isai and factorSweeps (tests/factor_isai_walk.py) must satisfy to pin
anything, on the CPU alone:

(a) the fixed-point sweeps reach the exact IC / ILU factor bit for bit and stay there.  With L forward levels that takes
    up to 2 L - 1 sweeps, not L: every entry comes from the values the sweep BEFORE left, so a row's off-diagonal entries
    wait one sweep for the pivots of the level below and its own pivot waits one more for them.  On the 4 x 3 x 3 box
    (8 levels) 8 sweeps are therefore not enough (asserted, so that the count is on record) and 15 are;
(b) W_L and W_U are inverses of the triangles on their own pattern: (W_L L) restricted to the pattern of W_L is the
    identity to 1e-13, and so is (U W_U) on the pattern of W_U for IC (W_U = W_L^T, U = L^T: the same statement transposed).
    ILU's W_U is generated row by row against U from the LEFT (w U(J, J) = e_0), so there it is (W_U U) that is the identity
    on the pattern; U W_U is not, on a graph with triangles;
(c) CG iterations on a Poisson box: BJ(1) > IC-isai p = 1 >= p = 2 >= exact IC, and a factor from 3 sweeps within one
    iteration of the exact factor's counts;
(d) the same for ILU under BiCGStab on the asymmetric random system."""
import numpy as np
import pytest

from ogl_amd import synthetic
from helpers import oracle_csr
import factor_isai_walk as fw
from test_gpu_incomplete_factor import factor_general, factor_pattern, levels

BOX = (4, 4, 4)  # (c): 23 / 19 / 15 / 13 iterations, strict (5^3 gives 29 / 21 / 16 / 16, 6^3 36 / 25 / 19 / 18)


@pytest.fixture(scope="module")
def random_csr(oracle):
    return oracle_csr(oracle, fw.random_system())


def test_random_system_has_triangles_and_a_repeated_column(random_csr):
    rp, cols, vals = random_csr
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    assert (np.diff(rows) == 0)[np.diff(cols) == 0].any()  # a cyclic face repeats a column
    frp, c, a, diag = factor_pattern(np.asarray(rp), np.asarray(cols), np.asarray(vals, float), True)
    assert sum(len(p) for p in fw.update_lists(frp, c, diag, True)) > 100  # triangles: IC's update list is not trivial


@pytest.mark.parametrize("kind", ["IC", "ILU"])
def test_sweeps_reach_the_exact_factor(oracle, kind):
    case = synthetic.poisson_block(4, 3, 3, symmetric=kind == "IC")
    rp, c, a, diag = factor_pattern(*[np.asarray(x) for x in oracle_csr(oracle, case)], kind == "IC")
    n_levels = len(levels(rp, c, False))
    assert n_levels == 8
    exact = factor_general(rp, c, a, diag, kind == "IC")
    need = next(s for s in range(1, 40) if np.array_equal(fw.swept_factor(rp, c, a, diag, kind == "IC", s), exact))
    print(kind, "sweeps to the exact factor:", need)
    assert n_levels < need <= 2 * n_levels - 1
    for s in (2 * n_levels - 1, 2 * n_levels + 2):  # reached, and a fixed point
        np.testing.assert_array_equal(fw.swept_factor(rp, c, a, diag, kind == "IC", s), exact)


def test_sweeps_reach_the_exact_factor_with_triangles(random_csr):
    rp0, cols, vals = random_csr
    for ic in (True, False):
        rp, c, a, diag = factor_pattern(np.asarray(rp0), np.asarray(cols), np.asarray(vals, float), ic)
        n_levels = len(levels(rp, c, False))
        np.testing.assert_array_equal(fw.swept_factor(rp, c, a, diag, ic, 2 * n_levels - 1),
                                      factor_general(rp, c, a, diag, ic))


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("kind", ["IC", "ILU"])
@pytest.mark.parametrize("system", ["box", "random"])
def test_w_is_the_inverse_on_its_pattern(oracle, random_csr, system, kind, power):
    if system == "box":
        csr = oracle_csr(oracle, synthetic.poisson_block(6, 5, 4, symmetric=kind == "IC"))
    else:
        csr = random_csr  # (IC: of its lower triangle, which is all IC reads)
    w = fw.Walk(oracle, *csr, kind, power=power)
    assert w.max_row <= fw.MAX_W_ROW
    WL, WU, L, U = (w.dense(k) for k in ("WL", "WU", "L", "U"))
    eye = np.eye(w.n)
    mask = WL != 0
    assert mask.sum() == w.w_entries
    assert np.abs((WL @ L - eye)[mask]).max() <= 1e-13
    if kind == "IC":  # W_U = W_L^T, U = L^T: U W_U = (W_L L)^T
        np.testing.assert_array_equal(WU, WL.T)
        assert np.abs((U @ WU - eye)[mask.T]).max() <= 1e-13
    else:  # rows of W_U are solved against U from the left
        assert np.abs((WU @ U - eye)[mask.T]).max() <= 1e-13


def iterations(oracle, csr, b, P, solver):
    A = oracle.DistMatrix(*csr)
    fn = oracle.cg if solver == "cg" else oracle.bicgstab
    res = fn(A, b, np.zeros_like(b), P, tolerance=1e-6, rel_tol=0.0, max_iter=500)
    assert res.final_residual <= 1e-6
    return res.n_iterations


def counts(oracle, csr, b, kind, solver):
    out = {"BJ": iterations(oracle, csr, b, oracle.jacobi_generate_scalar(*csr), solver)}
    for name, kw in (("p1", dict(power=1)), ("p2", dict(power=2)), ("exact", dict(isai=False)),
                     ("p1s3", dict(power=1, sweeps=3)), ("p2s3", dict(power=2, sweeps=3)),
                     ("exacts3", dict(isai=False, sweeps=3))):
        w = fw.Walk(oracle, *csr, kind, **kw)
        out[name] = iterations(oracle, csr, b, oracle.CallbackPrecond(w.apply), solver)
    return out


def test_cg_iteration_order(oracle):
    case = synthetic.poisson_block(*BOX)
    b, _ = synthetic.rhs_for_x_star(case)
    it = counts(oracle, oracle_csr(oracle, case), b, "IC", "cg")
    print(it)
    assert it["BJ"] > it["p1"] >= it["p2"] >= it["exact"], it
    assert it["BJ"] > it["p1"] > it["p2"] > it["exact"], it  # (strict on this box: it can tell the legs apart)
    for leg in ("p1", "p2", "exact"):
        assert abs(it[leg + "s3"] - it[leg]) <= 1, it


def test_bicgstab_iteration_order_ilu(oracle, random_csr):
    n = len(random_csr[0]) - 1
    b = np.random.default_rng(5).uniform(-1, 1, n)
    it = counts(oracle, random_csr, b, "ILU", "bicgstab")
    print(it)
    assert it["BJ"] > it["p1"] >= it["p2"] >= it["exact"], it
    for leg in ("p1", "p2", "exact"):
        assert abs(it[leg + "s3"] - it[leg]) <= 1, it
