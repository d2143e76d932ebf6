"""orc_precond_apply (Precond.apply): the apply inside every oracle solve, exported so that a device preconditioner can be
compared with it directly.  Pinned here against plain numpy: block Jacobi is the block inverses times r, ISAI(spd) is
W^T (W r), GISAI is W r, scalar Jacobi is r times the inverse diagonal."""
import numpy as np
import pytest
import scipy.sparse as sp

from ogl_amd import synthetic
from helpers import oracle_csr

RTOL = 1e-13


def system(oracle, symmetric=True, n=9):
    rp, cols, vals = oracle_csr(oracle, synthetic.poisson_case(n, symmetric=symmetric))
    r = np.random.default_rng(3).standard_normal(len(rp) - 1)
    return rp, cols, vals, r


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_block_jacobi_apply_is_the_block_inverses_times_r(oracle, k):
    rp, cols, vals, r = system(oracle, symmetric=False)
    A = sp.csr_matrix((vals, cols, rp)).toarray()
    P = oracle.Precond(rp, cols, vals, k)
    bp = P.block_ptrs if k > 1 else np.arange(len(r) + 1)
    want = np.empty_like(r)
    for b0, b1 in zip(bp[:-1], bp[1:]):
        want[b0:b1] = np.linalg.inv(A[b0:b1, b0:b1]) @ r[b0:b1]
    np.testing.assert_allclose(P.apply(r), want, rtol=RTOL, atol=0)
    if k > 1:
        assert np.diff(bp).max() > 1


@pytest.mark.parametrize("symmetric,isai", [(True, "spd"), (False, "general")])
def test_isai_apply_is_w_products(oracle, symmetric, isai):
    rp, cols, vals, r = system(oracle, symmetric=symmetric)
    P = oracle.Precond(rp, cols, vals, isai=isai)
    n = len(r)
    W = sp.csr_matrix((P.w_vals[:P.w_rowptr[-1]], P.w_cols[:P.w_rowptr[-1]], P.w_rowptr), shape=(n, n))
    want = W.T @ (W @ r) if isai == "spd" else W @ r
    np.testing.assert_allclose(P.apply(r), want, rtol=RTOL, atol=0)
    # W is the approximate inverse it claims to be: rows of W A (spd: of W A W^T) are e_i on W's pattern
    A = sp.csr_matrix((vals, cols, rp), shape=(n, n))
    if isai == "general":
        WA = (W @ A).toarray()
        i, j = W.nonzero()
        np.testing.assert_allclose(WA[i, j], (i == j).astype(float), atol=1e-12)


def test_identity_and_scalar_apply(oracle):
    rp, cols, vals, r = system(oracle)
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    P = oracle.Precond(rp, cols, vals, 1)
    np.testing.assert_array_equal(P.apply(r), r * inv)
    d = sp.csr_matrix((vals, cols, rp)).diagonal()
    np.testing.assert_allclose(P.apply(r), r / d, rtol=RTOL, atol=0)
