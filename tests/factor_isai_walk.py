"""The contract of the keywords `triangularSolves isai` and `factorSweeps N` of IC / ILU / IRILU as a
Python/NumPy walk, every product, difference and quotient rounded once:

* swept_factor: the factor from N synchronous fixed-point sweeps (every entry of sweep s from the values sweep s - 1 left);
* w_pattern / w_lower / w_upper: the approximate inverses W_L, W_U of the two triangles on the p-th power of the factor's
  lower-triangle pattern (W_U: its transpose), by substitution over each row's pattern;
* Walk.apply: z = W_U (W_L r), the rows summed through the oracle's SpMV (from 0, ascending column).

Shared by tests/test_factor_isai_walk.py (CPU) and tests/test_gpu_factor_isai.py and its worker (GPU).  The exact factor
comes from tests/test_gpu_incomplete_factor.py (factor_pattern, factor_general), unchanged."""
import math

import numpy as np

from test_gpu_incomplete_factor import Ref as ExactRef, factor_general, factor_pattern

MAX_W_ROW = 32


def _nan_sqrt(s):
    return math.sqrt(s) if s >= 0 else float("nan")


def _div(a, b):
    return float(np.float64(a) / np.float64(b))  # (IEEE: x / 0 and 0 / 0 without an exception)


def update_lists(rp, c, diag, ic):
    """Per factor entry e = (i, j) the pairs (pos(i, k), pos(k, j)) of its update, k ascending.
    IC: strictly lower entries, k < j common to rows i and j.  ILU: every entry, k < min(i, j)."""
    n = len(rp) - 1
    c = [int(x) for x in c]
    pairs = [[] for _ in range(len(c))]
    for i in range(n):
        where = {c[e]: e for e in range(rp[i], rp[i + 1])}
        if ic:
            for e in range(rp[i], diag[i]):
                j = c[e]
                for q in range(rp[j], diag[j]):
                    if c[q] in where:
                        pairs[e].append((where[c[q]], q))
        else:
            for e in range(rp[i], diag[i]):  # k = c[e] ascending
                k = c[e]
                for q in range(diag[k] + 1, rp[k + 1]):
                    if c[q] in where:
                        pairs[where[c[q]]].append((e, q))
    return pairs


def swept_factor(rp, c, a, diag, ic, sweeps):
    """The factor values after `sweeps` >= 1 synchronous sweeps from the start values (any number: the keyword caps it)."""
    assert sweeps >= 1
    n = len(rp) - 1
    rp, diag = [int(x) for x in rp], [int(x) for x in diag]
    c = [int(x) for x in c]
    a = [float(x) for x in a]
    pairs = update_lists(rp, c, diag, ic)
    v = [0.0] * len(a)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = diag[i]
            if ic:
                for e in range(rp[i], d):
                    v[e] = _div(a[e], _nan_sqrt(a[diag[c[e]]]))
                v[d] = _nan_sqrt(a[d])
            else:
                for e in range(rp[i], d):
                    v[e] = _div(a[e], a[diag[c[e]]])
                for e in range(d, rp[i + 1]):
                    v[e] = a[e]
        for _ in range(sweeps):
            new = [0.0] * len(a)
            for i in range(n):
                d = diag[i]
                if ic:
                    for e in range(rp[i], d):
                        s = a[e]
                        for pa, pb in pairs[e]:
                            s = s - v[pa] * v[pb]
                        new[e] = _div(s, v[diag[c[e]]])
                    s = a[d]
                    for e in range(rp[i], d):
                        s = s - v[e] * v[e]
                    new[d] = _nan_sqrt(s)
                else:
                    for e in range(rp[i], rp[i + 1]):
                        s = a[e]
                        for pa, pb in pairs[e]:
                            s = s - v[pa] * v[pb]
                        new[e] = _div(s, v[diag[c[e]]]) if e < d else s
            v = new
    return np.array(v)


def breakdown_row(rp, v, diag, ic):
    """The smallest row whose l_ii is not > 0 (IC) / whose u_ii is 0 or not finite (ILU); -1: none."""
    for i, d in enumerate(diag):
        x = v[d]
        if (not x > 0.0) if ic else (x == 0.0 or not math.isfinite(x)):
            return i
    return -1


def w_pattern(rp, c, diag, power):
    """Rows of W_L: the power-th power of the factor's lower-triangle pattern, the diagonal included, ascending."""
    n = len(rp) - 1
    low = [set(int(x) for x in c[rp[i]:diag[i] + 1]) for i in range(n)]
    rows = []
    for i in range(n):
        row = set(low[i])
        for _ in range(power - 1):
            nxt = set(row)
            for j in row:
                nxt |= low[j]
            row = nxt
        rows.append(sorted(row))
    return rows


def w_lower(rp, c, v, diag, rows, unit):
    """Row i of W_L over J = rows[i] (J[-1] = i), from the diagonal down."""
    c = [int(x) for x in c]
    entry = [{c[e]: e for e in range(rp[i], diag[i])} for i in range(len(rows))]
    out = []
    for i, J in enumerate(rows):
        m = len(J)
        assert J[-1] == i
        w = [0.0] * m
        for t in range(m - 1, -1, -1):
            s = 1.0 if t == m - 1 else 0.0
            for q in range(t + 1, m):
                e = entry[J[q]].get(J[t])
                if e is not None:
                    s = s - w[q] * v[e]
            w[t] = s if unit else _div(s, v[diag[J[t]]])
        out.append(w)
    return out


def w_upper(rp, c, v, diag, rows_t):
    """Row i of W_U (ILU) over J = rows_t[i] (J[0] = i), from the diagonal up."""
    c = [int(x) for x in c]
    entry = [{c[e]: e for e in range(diag[i] + 1, rp[i + 1])} for i in range(len(rows_t))]
    out = []
    for i, J in enumerate(rows_t):
        assert J[0] == i
        w = [0.0] * len(J)
        for t in range(len(J)):
            s = 1.0 if t == 0 else 0.0
            for q in range(t):
                e = entry[J[q]].get(J[t])
                if e is not None:
                    s = s - w[q] * v[e]
            w[t] = _div(s, v[diag[J[t]]])
        out.append(w)
    return out


def to_csr(rows, vals):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.array([j for r in rows for j in r], np.int64)
    v = np.array([x for r in vals for x in r], np.float64)
    return rp, cols, v


def transpose_rows(rows):
    """Pattern of the transpose, rows ascending, with the (row, slot) each entry comes from."""
    n = len(rows)
    t_rows, src = [[] for _ in range(n)], [[] for _ in range(n)]
    for i, J in enumerate(rows):
        for t, j in enumerate(J):
            t_rows[j].append(i)
            src[j].append((i, t))
    return t_rows, src


class Walk:
    """The preconditioner of one local matrix (rowptr, cols, vals in the caller's numbering) under the two keywords.
    kind: IC | ILU | IRILU; isai: triangularSolves isai with sparsityPower `power`; sweeps: factorSweeps (0: the exact
    factor)."""

    def __init__(self, oracle, rowptr, cols, vals, kind, isai=True, power=1, sweeps=0):
        ic = kind == "IC"
        self.oracle, self.kind, self.ic, self.isai = oracle, kind, ic, isai
        rp, c, a, diag = factor_pattern(np.asarray(rowptr), np.asarray(cols), np.asarray(vals, np.float64), ic)
        self.rp, self.c, self.diag, self.n = rp, c, diag, len(rp) - 1
        self.a = a
        with np.errstate(all="ignore"):
            self.v = swept_factor(rp, c, a, diag, ic, sweeps) if sweeps else factor_general(rp, c, a, diag, ic)
        self.breakdown = breakdown_row(rp, self.v, diag, ic)
        if not isai:  # the exact solves / IRILU's sweeps on this factor
            self.exact = ExactRef.__new__(ExactRef)
            self._fill_exact(kind)
            return
        assert kind != "IRILU"
        self.rows = w_pattern(rp, c, diag, power)
        self.w_entries = sum(len(r) for r in self.rows)
        self.max_row = max(len(r) for r in self.rows)
        with np.errstate(all="ignore"):
            wl = w_lower(rp, c, self.v, diag, self.rows, unit=not ic)
            self.rows_t, src = transpose_rows(self.rows)
            if ic:  # W_U = W_L^T, gathered
                wu = [[wl[i][t] for i, t in s] for s in src]
            else:
                wu = w_upper(rp, c, self.v, diag, self.rows_t)
        self.WL = to_csr(self.rows, wl)
        self.WU = to_csr(self.rows_t, wu)

    def _fill_exact(self, kind):
        """An ExactRef (test_gpu_incomplete_factor.Ref) around this object's factor values."""
        from test_gpu_incomplete_factor import levels
        e, rp, c, diag = self.exact, self.rp, self.c, self.diag
        e.kind, e.ic, e.rp, e.c, e.diag, e.n, e.v = kind, self.ic, rp, c, diag, self.n, self.v
        e.fwd = levels(rp, c, False)
        if self.ic:
            n = self.n
            rows = np.repeat(np.arange(n), np.diff(rp))
            order = np.lexsort((rows, c))
            e.trp = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))])
            e.tc, e.tv = rows[order], self.v[order]
            e.ubeg, e.uend, e.uc, e.uv = e.trp[:-1], e.trp[1:], e.tc, e.tv
        else:
            e.ubeg, e.uend, e.uc, e.uv = diag, rp[1:], c, self.v
        e.bwd = levels(np.concatenate([[0], np.cumsum(e.uend - e.ubeg)]),
                       np.concatenate([e.uc[a:b] for a, b in zip(e.ubeg, e.uend)]), True) if kind != "IRILU" else None

    def apply(self, r):
        r = np.ascontiguousarray(r, np.float64)
        if not self.isai:
            with np.errstate(all="ignore"):
                return self.exact.apply(r)
        y = self.oracle.spmv(*self.WL, r)
        return self.oracle.spmv(*self.WU, y)

    def dense(self, which):
        """W_L | W_U | L | U as dense arrays (the CPU checks)."""
        n = self.n
        out = np.zeros((n, n))
        if which in ("WL", "WU"):
            rp, c, v = self.WL if which == "WL" else self.WU
            rows = np.repeat(np.arange(n), np.diff(rp))
            out[rows, c] = v
            return out
        rows = np.repeat(np.arange(n), np.diff(self.rp))
        low = self.c <= rows if which == "L" else self.c >= rows
        if self.ic:  # the factor holds L; U = L^T
            out[rows, self.c] = self.v
            return out if which == "L" else out.T
        out[rows[low], self.c[low]] = self.v[low]
        if which == "L":
            out[np.arange(n), np.arange(n)] = 1.0
        return out


def random_system(n=650, seed=11, hub=None):
    """One asymmetric random lduMatrix system as tests/test_gpu_random_systems.py draws them: faces within a window of 6
    rows (triangles in the graph), a cyclic patch pair whose first face repeats a column of the matrix, diagonally
    dominant.  hub: a row coupled to that many earlier rows (a wide row of W at sparsityPower 2)."""
    from ogl_amd import synthetic
    rng = np.random.default_rng(seed)
    pairs = set()
    for i in range(n - 1):
        for j in rng.integers(i + 1, min(n, i + 7), 3):
            pairs.add((i, int(j)))
    if hub:
        for i in range(hub):
            pairs.add((3 * i, n - 1))
    pairs = np.array(sorted(pairs), dtype=np.int32).reshape(-1, 2)
    f = len(pairs)
    upper, lower = rng.uniform(-1, 0, f), rng.uniform(-1, 0, f)
    m = 6
    a = rng.choice(n, m, replace=False).astype(np.int32)
    b = rng.choice(n, m, replace=False).astype(np.int32)
    a[0], b[0] = pairs[f // 2]
    ifaces = [synthetic.Interface(synthetic.IFACE_CYCLIC, a, rng.uniform(0, 0.5, m), -1, 1),
              synthetic.Interface(synthetic.IFACE_CYCLIC, b, rng.uniform(0, 0.5, m), -1, 0)]
    diag = np.full(n, 1.0)
    np.add.at(diag, pairs[:, 0], np.abs(upper))
    np.add.at(diag, pairs[:, 1], np.abs(lower))
    for itf in ifaces:
        np.add.at(diag, itf.face_cells, np.abs(itf.bou_coeffs))
    return synthetic.LduCase(n, pairs[:, 0].copy(), pairs[:, 1].copy(), diag, upper, lower, ifaces)
