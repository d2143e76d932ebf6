"""The drawn systems of tests/random_precond_cases.py, without a device: the conditions the list must meet to pin anything
(sizes around the chunk edges, both symmetries, cyclic pairs, few refusals), the soundness of every reference solve the GPU
tests compare with, and one negative control per comparison helper of tests/test_gpu_random_preconds.py -- the helper is
handed what a device following the right reference would leave and a reference that is wrong in one place, and must raise."""
import copy

import numpy as np
import pytest

import chebyshev_walk as cw
import factor_isai_walk as fw
import mixed_walk as mw
import random_precond_cases as rc
import test_gpu_random_preconds as dev

ALL = list(range(rc.N_CASES))


def test_the_list_is_stratified():
    C = rc.chunk_rows()
    ps = [rc.params(i) for i in ALL]
    n = np.array([p.n for p in ps])
    assert len(ps) == 48
    assert (n > C).sum() >= 12 and (n > 2 * C).sum() >= 6 and (n <= 4).sum() >= 6, n
    assert n.min() == 2 and n.max() <= 2 * C + 80
    for size in rc.fixed_sizes():
        assert size in n, size
    sym = sum(p.symmetric for p in ps)
    assert sym >= 20 and len(ps) - sym >= 20
    assert sum(p.cyclic for p in ps) >= 20
    assert {p.reach for p in ps} == set(rc.REACHES) and {p.per_row for p in ps} == {1, 2, 3, 4, 5}
    # every case is what its parameters say, and the same when built again
    for i in ALL:
        c = rc.case(i)
        assert c.ldu.n_cells == c.params.n and c.ldu.symmetric == c.params.symmetric
        assert bool(c.ldu.interfaces) == c.params.cyclic
        assert (c.ldu.upper_addr - c.ldu.lower_addr).max() <= c.params.reach
    again = rc._drawn(rc.params(17))
    np.testing.assert_array_equal(again.upper, rc.case(17).ldu.upper)
    np.testing.assert_array_equal(again.upper_addr, rc.case(17).ldu.upper_addr)


def test_what_a_case_is_factorised_and_solved_with_is_not_tied_to_its_pattern():
    """reach x sweeps (i % 3), per_row x degree (i % 5), solver x sweeps, numbering x symmetry: every pair occurs."""
    ps = [rc.params(i) for i in ALL]
    assert len({(p.reach, i % 3) for i, p in enumerate(ps)}) == 9
    assert len({(p.per_row, i % 5) for i, p in enumerate(ps)}) == 25
    assert len({(p.solver == "gmres", i % 3) for i, p in enumerate(ps)}) == 6
    assert len({(p.renumber, p.symmetric, p.cyclic) for p in ps}) == 8
    assert sum(p.solver == "gmres" for p in ps) >= 12
    for size in rc.fixed_sizes()[2:]:  # (from 63 rows on: each fixed size in both symmetries, renumbered and not)
        seen = {(p.symmetric, p.renumber) for p in ps if p.n == size}
        assert len(seen) == 2, (size, seen)


def test_the_edges_are_what_they_are_named():
    C = rc.chunk_rows()
    assert rc.case("one_row").ldu.n_cells == 1 and rc.case("one_row").ldu.n_faces == 0
    for name in ("diagonal5_sym", "diagonal5_asym"):
        c = rc.case(name)
        assert c.ldu.n_cells == 5 and c.ldu.n_faces == 0 and c.ldu.symmetric == (name == "diagonal5_sym")
    for name in rc.HUBS:
        rp = rc.case(name).csr[0]
        assert np.diff(rp).max() == rc.HUB_WIDTH + 2 > 64  # (wider than a wavefront)
        w = rc.reference("ILU_isai_p1", name)
        assert max(len(r) for r in w.rows) <= 3 and max(len(r) for r in w.rows_t) == rc.HUB_WIDTH + 2
    for name in ("chain_sym", "chain_asym"):
        c = rc.case(name)
        assert c.ldu.n_cells == C + 1
        assert dev.facts_of("ILU", name, rc.reference("ILU", name))["iluLevels"] == C + 1  # a level per row


@pytest.mark.parametrize("power,variants", [(1, ("IC_isai_p1", "ILU_isai_p1")), (2, ("IC_isai_p2", "ILU_isai_p2"))])
def test_few_cases_are_refused(power, variants):
    """Refused: exactly where a row of W_L or of W_U is wider than the device's 32; at most 1 case in 10."""
    keys = ALL if power == 1 else [i for i in ALL if rc.narrow(i)]
    assert len(keys) >= 8
    for variant in variants:
        mine = [k for k in keys if rc.accepts(variant, k)]
        assert mine == [k for k in ALL if rc.accepts(variant, k)]
        refused = [k for k in mine if rc.too_wide(variant, k)]
        print(variant, "cases", len(mine), "refused", refused, "widest",
              max(rc.w_width(rc.reference(variant, k)) for k in mine))
        assert 10 * len(refused) <= len(mine), (variant, refused)
    # (over the whole list, as the issue counts: the ILU form runs on every case)
    assert 10 * sum(rc.too_wide(variants[1], k) for k in keys) <= len(keys)


@pytest.mark.parametrize("variant", [v for v in rc.VARIANTS if rc.VARIANTS[v][1].get("fused", 1) and
                                     "stream" not in rc.VARIANTS[v][1] and "force_layout" not in rc.VARIANTS[v][1]])
def test_the_reference_solves_are_sound(variant):
    """tolerance 1e-12, maxIter 12 with the reference called back: a finite history whose last entry is below its first, in
    the numbering the library gives the device copy.  (The Chebyshev variants share one reference: cheb_fused stands for all.)"""
    ran = 0
    for key in ALL + list(rc.EDGES):
        if not rc.accepts(variant, key) or rc.too_wide(variant, key):
            continue
        new_id = rc.host_numbering(key)
        assert (new_id is not None) == rc.params_of(key).renumber, rc.describe(key)
        out = rc.oracle_solve(variant, key, new_id)
        h = out.history
        assert np.isfinite(h).all() and np.isfinite(out.x).all(), (variant, rc.describe(key))
        assert len(h) >= 2 and h[-1] < h[0], (variant, rc.describe(key), h)
        if variant == "mg_single":
            assert rc.reference(variant, key).smallest_fp32 >= mw.TINY32, rc.describe(key)
        ran += 1
    assert ran >= 6  # (the fewest: IC at sparsityPower 2, four narrow symmetric cases and three edges)


def test_chebyshev_on_a_diagonal_matrix_is_the_polynomial_at_one():
    for name in ("diagonal5_sym", "diagonal5_asym"):
        c = rc.case(name)
        w = rc.reference("cheb_fused", name)
        assert w.table.lambda_max == 1.0 and rc.degree_of(name) == 4
        q = float(w.polynomial(1.0))
        assert abs(q - 1.3079) < 1e-4, q
        np.testing.assert_allclose(w.apply(c.r), q * c.r / c.ldu.diag, rtol=1e-14)


# ---- negative controls: a comparison that passed against a wrong reference would be worthless ----
KEY = 20  # 1,025 rows, symmetric, not renumbered: one row in the third chunk


def last_chunk_row(key):
    n = rc.params_of(key).n
    assert n > 2 * rc.chunk_rows()
    return n - 1


def test_a_factor_value_one_ulp_off_is_noticed():
    variant = "ILU"
    right = rc.reference(variant, KEY)
    got = dev.FromReference(variant, KEY)
    dev.check_factor(got, right, variant, KEY)  # (and the right one compares equal)
    wrong = copy.copy(right)
    wrong.v = right.v.copy()
    e = right.diag[last_chunk_row(KEY)]
    wrong.v[e] = np.nextafter(wrong.v[e], np.inf)
    wrong.uv = wrong.v
    with pytest.raises(AssertionError, match="z = M\\^-1 r"):
        dev.check_factor(got, wrong, variant, KEY)


def test_a_dropped_entry_of_w_is_noticed():
    variant = "IC_isai_p1"
    right = rc.reference(variant, KEY)
    got = dev.FromReference(variant, KEY)
    dev.check_isai(got, right, variant, KEY)
    rp, cols, vals = right.WL
    row = last_chunk_row(KEY)
    e = int(rp[row])
    assert rp[row + 1] - e >= 2 and cols[e] != row  # (an off-diagonal entry of the last row)
    wrong = copy.copy(right)
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    wrong.WL = (rp2, np.delete(cols, e), np.delete(vals, e))
    with pytest.raises(AssertionError, match="z = M\\^-1 r"):
        dev.check_isai(got, wrong, variant, KEY)  # (the count of the pattern left as it was: the values alone show it)
    wrong.w_entries = right.w_entries - 1
    with pytest.raises(AssertionError, match="triangularWEntries"):
        dev.check_isai(got, wrong, variant, KEY)


def test_one_degree_more_is_noticed():
    variant = "cheb_unfused"
    right = rc.reference(variant, KEY)
    got = dev.FromReference(variant, KEY)
    dev.check_chebyshev(got, right, variant, KEY)
    wrong = cw.Walk(rc._oracle(), *rc.case(KEY).csr, degree=rc.degree_of(KEY) + 1)
    assert wrong.table.lambda_max == right.table.lambda_max  # (the bounds agree: the apply shows it)
    with pytest.raises(AssertionError, match="z = M\\^-1 r"):
        dev.check_chebyshev(got, wrong, variant, KEY)


@pytest.mark.parametrize("variant", ["mg_double", "mg_single"])
def test_a_reassigned_aggregate_is_noticed(variant):
    right = rc.reference(variant, KEY)
    got = dev.FromReference(variant, KEY)
    dev.check_multigrid(got, right, variant, KEY)
    h = dev.hierarchy_of(right)
    wrong_h = copy.copy(h)
    wrong_h.agg = [a.copy() for a in h.agg]
    row = last_chunk_row(KEY)
    wrong_h.agg[0][row] = (h.agg[0][row] + 1) % h.A[1].n
    wrong = wrong_h
    if variant == "mg_single":
        wrong = copy.copy(right)
        wrong.ref = wrong_h
    with pytest.raises(AssertionError, match="agg of level 0"):
        dev.check_multigrid(got, wrong, variant, KEY)
