"""Preconditioners IC, ILU and IRILU (factorization::Ic / Ilu, Ilu<Ir, Ir>; Preconditioner.H:106-126,147-178) against a
reference of the contract in this file: IC(0) / ILU(0) of the local matrix in the caller's numbering, rows ascending,
entries in ascending column, products and sums rounded separately -- the device's z = M^-1 r must carry the same bits."""
import copy
import math

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import oracle_csr

pytestmark = pytest.mark.gpu

KINDS = {"IC": capi.PRECOND_IC, "ILU": capi.PRECOND_ILU, "IRILU": capi.PRECOND_IRILU}
SWEEPS = 5


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def factor_pattern(rowptr, cols, vals, ic):
    """(rp, c, v, diag) of the factor's CSR: a repeated column is one entry (sum in stored order), IC keeps tril."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    keep = cols <= rows if ic else np.ones(len(cols), bool)
    r, c, v = rows[keep], cols[keep], vals[keep]
    first = np.ones(len(c), bool)
    first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    if not first.all():  # (cyclic patches: sum the repeats in stored order)
        out = []
        for k in range(len(c)):
            if first[k]:
                out.append(v[k])
            else:
                out[-1] = out[-1] + v[k]
        v = np.array(out)
        r, c = r[first], c[first]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    rp = np.cumsum(rp)
    diag = np.flatnonzero(c == r)
    assert len(diag) == n
    return rp, c.astype(np.int64), v.astype(np.float64).copy(), diag


def levels(rp, c, upper):
    """Level of every row over the strictly lower (upper) entries: a fixed point, any valid schedule gives the same
    bits.  Returns the rows of each level, in processing order."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    m = c > rows if upper else c < rows
    dep_r, dep_c = rows[m], c[m]
    lev = np.zeros(n, np.int64)
    starts = np.flatnonzero(np.r_[True, dep_r[1:] != dep_r[:-1]]) if len(dep_r) else np.zeros(0, np.int64)
    while True:
        cand = np.zeros(n, np.int64)
        if len(dep_r):
            cand[dep_r[starts]] = np.maximum.reduceat(lev[dep_c] + 1, starts)
        if np.array_equal(cand, lev):
            break
        lev = cand
    order = np.argsort(lev, kind="stable")
    bounds = np.searchsorted(lev[order], np.arange(lev.max() + 2))
    return [order[bounds[k]:bounds[k + 1]] for k in range(len(bounds) - 1)]


def factor_general(rp, c, v, diag, ic):
    """The contract's row loop (small cases)."""
    v = v.tolist()
    n = len(rp) - 1
    c = c.tolist()
    for i in range(n):
        where = {c[e]: e for e in range(rp[i], rp[i + 1])}
        d = diag[i]
        for e in range(rp[i], d):
            k = c[e]
            if ic:
                s = v[e]
                for q in range(rp[k], diag[k]):
                    if c[q] in where:
                        s = s - v[where[c[q]]] * v[q]
                v[e] = s / v[diag[k]]
            else:
                l_ = v[e] / v[diag[k]]
                v[e] = l_
                for q in range(diag[k] + 1, rp[k + 1]):
                    if c[q] in where:
                        p = where[c[q]]
                        v[p] = v[p] - l_ * v[q]
        if ic:
            s = v[d]
            for e in range(rp[i], d):
                s = s - v[e] * v[e]
            v[d] = math.sqrt(s) if s >= 0 else float("nan")
    return np.array(v)


def factor_no_triangles(rp, c, v, diag, ic, lev):
    """The same, vectorised per level, for graphs without triangles (7-point stencils): the only update of row i is
    its diagonal's."""
    v = v.copy()
    n = len(rp) - 1
    for rows in lev:
        lo, d = rp[rows], diag[rows]
        cnt = d - lo
        acc = v[d].copy()
        for t in range(int(cnt.max()) if len(rows) else 0):
            m = t < cnt
            e = lo[m] + t
            k = c[e]
            if ic:
                v[e] = v[e] / v[diag[k]]
                acc[m] = acc[m] - v[e] * v[e]
            else:
                v[e] = v[e] / v[diag[k]]
                pos = _find(rp, c, k, rows[m])  # u_ki: the entry of row k at column i
                acc[m] = acc[m] - v[e] * v[pos]
        v[d] = np.sqrt(acc) if ic else acc
    return v


def _find(rp, c, rows, cols):
    """position of (rows[t], cols[t]) in the CSR (row segments are sorted)."""
    out = np.empty(len(rows), np.int64)
    lo, hi = rp[rows].copy(), rp[rows + 1].copy()
    while True:  # vectorised binary search
        act = lo < hi
        if not act.any():
            break
        mid = (lo + hi) // 2
        less = np.zeros(len(rows), bool)
        less[act] = c[mid[act]] < cols[act]
        lo = np.where(act & less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)
    out[:] = lo
    assert np.array_equal(c[out], cols)
    return out


class Ref:
    def __init__(self, rowptr, cols, vals, kind, general):
        ic = kind == "IC"
        self.kind, self.ic = kind, ic
        rp, c, v, diag = factor_pattern(np.asarray(rowptr), np.asarray(cols), np.asarray(vals, np.float64), ic)
        self.rp, self.c, self.diag, self.n = rp, c, diag, len(rp) - 1
        self.fwd = levels(rp, c, False)
        self.v = factor_general(rp, c, v, diag, ic) if general else factor_no_triangles(rp, c, v, diag, ic, self.fwd)
        if ic:  # L^T by rows, diagonal first
            n = self.n
            rows = np.repeat(np.arange(n), np.diff(rp))
            order = np.lexsort((rows, c))
            self.trp = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))])
            self.tc, self.tv = rows[order], self.v[order]
            self.ubeg, self.uend, self.uc, self.uv = self.trp[:-1], self.trp[1:], self.tc, self.tv
        else:
            self.ubeg, self.uend, self.uc, self.uv = diag, rp[1:], c, self.v
        self.bwd = levels(np.concatenate([[0], np.cumsum(self.uend - self.ubeg)]),
                          np.concatenate([self.uc[a:b] for a, b in zip(self.ubeg, self.uend)]) if self.n else c,
                          True) if kind != "IRILU" else None

    def _lower(self, b):
        x = np.zeros(self.n)
        for rows in self.fwd:
            lo, hi = self.rp[rows], self.diag[rows]
            s = b[rows].copy()
            cnt = hi - lo
            for t in range(int(cnt.max()) if len(rows) else 0):
                m = t < cnt
                e = lo[m] + t
                s[m] = s[m] - self.v[e] * x[self.c[e]]
            x[rows] = s / self.v[hi] if self.ic else s
        return x

    def _upper(self, y):
        x = np.zeros(self.n)
        for rows in self.bwd:
            d, hi = self.ubeg[rows], self.uend[rows]
            s = y[rows].copy()
            cnt = hi - d - 1
            for t in range(int(cnt.max()) if len(rows) else 0):
                m = t < cnt
                e = d[m] + 1 + t
                s[m] = s[m] - self.uv[e] * x[self.uc[e]]
            x[rows] = s / self.uv[d]
        return x

    def _sweep(self, upper, b, x):
        n = self.n
        s = b.copy()
        if upper:
            d, hi = self.diag, self.rp[1:]
            s = s - self.v[d] * x
            lo = d + 1
        else:
            lo, hi = self.rp[:-1], self.diag
        cnt = hi - lo
        for t in range(int(cnt.max()) if n else 0):
            m = t < cnt
            e = lo[m] + t
            s[m] = s[m] - self.v[e] * x[self.c[e]]
        if upper:
            return x + s * (1.0 / self.v[self.diag])
        s = s - x
        return x + s

    def apply(self, r):
        r = np.asarray(r, np.float64)
        if self.kind == "IRILU":
            x = r
            for _ in range(SWEEPS):
                x = self._sweep(False, r, x)
            y = x
            for _ in range(SWEEPS):
                x = self._sweep(True, y, x)
            return x
        return self._upper(self._lower(r))


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
def cfg(kind, solver=capi.SOLVER_CG, **kw):
    base = dict(solver=solver, preconditioner=KINDS[kind], tolerance=1e-8, rel_tol=0.0, max_iter=2000,
                renumber=capi.RENUMBER_OFF)
    base.update(kw)
    return capi.default_config(**base)


def device_apply(reg, name, case, kind, r, **kw):
    s = reg.solver(name, cfg(kind, **kw)).set_matrix(case)
    b = np.ones(case.n_cells)
    s.solve(b, np.zeros(case.n_cells))
    return s, s.apply_preconditioner(r)


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


def check_bits(oracle, reg, name, case, kinds=("IC", "ILU", "IRILU"), general=True, **kw):
    rowptr, cols, vals = oracle_csr(oracle, case)
    r = rhs(case.n_cells)
    for kind in kinds:
        if kind == "IC" and not case.symmetric:
            continue
        ref = Ref(rowptr, cols, vals, kind, general)
        s, z = device_apply(reg, f"{name}_{kind}", case, kind, r, **kw)
        np.testing.assert_array_equal(z, ref.apply(r), err_msg=f"{name} {kind}")
        assert s.get_property("iluBreakdownRow") == -1.0


CASES = {
    "poisson_sym": lambda: synthetic.poisson_case(12),
    "poisson_asym": lambda: synthetic.poisson_case(12, symmetric=False),
    "voronoi": lambda: synthetic.voronoi_case(3000),
    "long_rows": lambda: synthetic.long_rows_case(synthetic.poisson_case(14), 0.2, 14),
    "periodic_x": lambda: synthetic.poisson_block(10, 8, 6, periodic_x=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_apply_bit_identical(oracle, name):
    reg = capi.Registry()
    check_bits(oracle, reg, name, CASES[name]())
    reg.close()


def test_apply_bit_identical_128(oracle):
    """128^3 in natural order (382 levels): the thin ends and the wide middle."""
    reg = capi.Registry()
    case = synthetic.poisson_case(128)
    check_bits(oracle, reg, "p128", case, general=False)
    s = reg.solver("p128_IC", cfg("IC"))
    assert s.get_property("iluLevels") == 3 * 128 - 2
    assert 2 <= s.get_property("iluLaunchesPerApply") < 2 * (3 * 128 - 2)
    reg.close()


@pytest.mark.parametrize("kind", ["IC", "ILU", "IRILU"])
def test_renumbered_equals_caller_numbering(kind):
    """The factor is that of the caller's numbering: with renumber on, z carries the same bits."""
    case = synthetic.renumber_case(synthetic.poisson_case(14), 4096)
    r = rhs(case.n_cells)
    reg = capi.Registry()
    _, z0 = device_apply(reg, "off_" + kind, case, kind, r, renumber=capi.RENUMBER_OFF)
    s1, z1 = device_apply(reg, "on_" + kind, case, kind, r, renumber=capi.RENUMBER_ON)
    assert s1.get_property("renumbered") == 1.0  # (the device copy really is in a numbering of its own)
    reg.close()
    np.testing.assert_array_equal(z1, z0)


@pytest.mark.parametrize("solver,kind", [(capi.SOLVER_CG, "IC"), (capi.SOLVER_BICGSTAB, "ILU"),
                                         (capi.SOLVER_GMRES, "IRILU")])
def test_solves_converge(solver, kind):
    case = synthetic.poisson_case(20, symmetric=kind == "IC")
    xs = synthetic.x_star(case.global_index, case.global_n)
    b = synthetic.apply_case(case, xs)
    reg = capi.Registry()
    s = reg.solver("solve_" + kind, cfg(kind, solver=solver, tolerance=1e-9)).set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    reg.close()
    assert 0 < perf.n_iterations < 2000 and perf.final_residual <= 1e-9, (perf.n_iterations, perf.final_residual)
    # the true residual, normalised as the criterion does (StoppingCriterion.H:136), meets the tolerance too
    true_res = np.abs(b - synthetic.apply_case(case, x)).sum() / perf.norm_factor
    assert true_res <= 2e-9, (true_res, perf.final_residual)
    assert np.abs(x - xs).max() < 1e-5


def test_ic_fewer_iterations_than_jacobi():
    case = synthetic.poisson_case(24)
    b = synthetic.apply_case(case, synthetic.x_star(case.global_index, case.global_n))
    reg = capi.Registry()
    its = {}
    for kind, pc in (("IC", capi.PRECOND_IC), ("BJ", capi.PRECOND_BJ)):
        c = capi.default_config(solver=capi.SOLVER_CG, preconditioner=pc, tolerance=1e-6, rel_tol=0.0, max_iter=2000)
        _, perf = reg.solver("it_" + kind, c).set_matrix(case).solve(b, np.zeros_like(b))
        its[kind] = perf.n_iterations
    reg.close()
    assert its["IC"] < its["BJ"], its


def test_values_refresh_gives_new_factor(oracle):
    case = synthetic.poisson_case(10, symmetric=False)
    r = rhs(case.n_cells)
    reg = capi.Registry()
    s = reg.solver("refresh", cfg("ILU")).set_matrix(case)
    s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    case2 = copy.copy(case)
    case2.diag = case.diag * 1.5
    s = reg.solver("refresh", cfg("ILU")).set_matrix(case2)
    s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    z = s.apply_preconditioner(r)
    reg.close()
    rowptr, cols, vals = oracle_csr(oracle, case2)
    np.testing.assert_array_equal(z, Ref(rowptr, cols, vals, "ILU", True).apply(r))


def test_caching_reuses_stored_factor(oracle):
    """caching 1: the second solve uses the stored object (the first matrix's factor), the third generates afresh."""
    case = synthetic.poisson_case(10)
    r = rhs(case.n_cells)
    reg = capi.Registry()
    c = cfg("IC", caching=1)
    zs = []
    cases = [case]
    for step in range(3):
        cs = copy.copy(case)
        cs.diag = case.diag * (1.0 + 0.25 * step)
        cases.append(cs)
        s = reg.solver("cache", c).set_matrix(cs)
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
        zs.append(s.apply_preconditioner(r))
    reg.close()
    ref = [Ref(*oracle_csr(oracle, cases[k + 1]), "IC", True).apply(r) for k in range(3)]
    np.testing.assert_array_equal(zs[0], ref[0])
    np.testing.assert_array_equal(zs[1], ref[0])  # stored
    np.testing.assert_array_equal(zs[2], ref[2])  # counter ran out: generated for this solve


def test_breakdown_is_reported():
    """A negative diagonal: IC's first pivot is not positive -- the solve fails naming IC and the row, no NaN psi."""
    case = synthetic.poisson_case(8)
    neg = copy.copy(case)
    neg.diag, neg.upper = -case.diag, -case.upper
    b = synthetic.apply_case(neg, synthetic.x_star(neg.global_index, neg.global_n))
    reg = capi.Registry()
    s = reg.solver("neg", cfg("IC")).set_matrix(neg)
    with pytest.raises(capi.OglError) as e:
        s.solve(b, np.zeros_like(b))
    assert e.value.status == capi.ERR_INVALID and "IC" in str(e.value) and "row 0" in str(e.value), e.value
    assert s.get_property("iluBreakdownRow") == 0.0
    s2 = reg.solver("neg_ilu", cfg("ILU", solver=capi.SOLVER_BICGSTAB)).set_matrix(neg)  # (ILU has no sign condition)
    x, perf = s2.solve(b, np.zeros_like(b))
    assert s2.get_property("iluBreakdownRow") == -1.0
    reg.close()
    assert perf.final_residual <= 1e-8 and np.isfinite(x).all()


def test_apply_before_solve_is_a_state_error():
    case = synthetic.poisson_case(4)
    reg = capi.Registry()
    s = reg.solver("early", cfg("ILU")).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.apply_preconditioner(np.ones(case.n_cells))
    reg.close()
    assert e.value.status == capi.ERR_STATE


def test_time_steps_leave_no_memory_behind():
    import soak_worker
    case = synthetic.poisson_case(16)
    b = np.ones(case.n_cells)
    reg = capi.Registry()
    marks = {}
    for step in range(10):
        case.diag[:] = case.diag * (1.0 + 1e-9)
        s = reg.solver("steps", cfg("IC")).set_matrix(case)
        s.solve(b, np.zeros_like(b))
        if step in (3, 9):
            marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[9][k] == marks[3][k], (k, marks)


def test_apply_after_another_field_regenerated_or_pattern_changed_is_a_state_error(oracle):
    """The registry-wide store is shared: a field whose stored object another field has since regenerated (another size),
    or whose pattern changed since its solve, has no preconditioner to apply until it solves again."""
    a, b = synthetic.poisson_case(8), synthetic.poisson_case(12)
    reg = capi.Registry()
    sa, _ = device_apply(reg, "field_a", a, "IC", rhs(a.n_cells))
    device_apply(reg, "field_b", b, "IC", rhs(b.n_cells))  # another n: generated into the shared slot
    with pytest.raises(capi.OglError) as e:
        sa.apply_preconditioner(rhs(a.n_cells))
    assert e.value.status == capi.ERR_STATE, e.value
    sa.solve(np.ones(a.n_cells), np.zeros(a.n_cells))  # solving again sets it up afresh
    np.testing.assert_array_equal(sa.apply_preconditioner(rhs(a.n_cells)),
                                  Ref(*oracle_csr(oracle, a), "IC", True).apply(rhs(a.n_cells)))
    c = synthetic.poisson_case(9)
    sa = reg.solver("field_a", cfg("IC")).set_matrix(c)  # a new pattern (and size) for the same field
    with pytest.raises(capi.OglError) as e:
        sa.apply_preconditioner(rhs(c.n_cells))
    reg.close()
    assert e.value.status == capi.ERR_STATE, e.value
