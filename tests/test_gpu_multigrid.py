"""Preconditioner Multigrid (Preconditioner.H:259-341) against a NumPy restatement of its contract in
this file: the aggregation hierarchy of the local matrix in the caller's numbering -- aggregates integer-exact, coarse
matrices bit for bit -- and one V-cycle as the apply, z = M^-1 r bit for bit.  Products and sums round separately; the
coarsest level's CG takes its dot products in the loop's reduction tree (oracle.dot under helpers.blocked)."""
import copy
import os
import sys

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OMEGA = 0.9
ROUNDS = 15
DEFAULTS = dict(maxLevels=9, minCoarseRows=10, coarseSolverIters=4)


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def seq_sums(starts, lens, terms, init=None):
    """out[g] = (((init[g] + t[s]) + t[s + 1]) + ...) over the run [starts[g], starts[g] + lens[g]) of `terms`, one
    rounding per sum; init None: the run's first term starts the sum."""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    if init is None:
        acc = terms[starts].astype(np.float64) if len(starts) else np.zeros(0)
        first = 1
    else:
        acc = np.array(init, np.float64)
        first = 0
    for t in range(first, int(lens.max()) if len(lens) else 0):
        m = t < lens
        acc[m] = acc[m] + terms[starts[m] + t]
    return acc


class Csr:
    def __init__(self, rp, cols, vals):
        self.rp, self.cols = np.asarray(rp, np.int64), np.asarray(cols, np.int64)
        self.vals = np.asarray(vals, np.float64)
        self.n = len(self.rp) - 1
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rp))

    def mul(self, x):
        """(A x)_i summed from 0 in stored (ascending column) order: the SpMV contract."""
        return seq_sums(self.rp[:-1], np.diff(self.rp), self.vals * x[self.cols], init=np.zeros(self.n))


def strongest(n, r, c, st, agg, want_aggregated):
    """s[i] for the unaggregated rows i: the neighbour (aggregated or not, as asked) of the largest strength, ties to the
    larger column; -1: none."""
    s = np.full(n, -1, np.int64)
    m = (agg[r] == -1) & ((agg[c] != -1) == want_aggregated)
    rr, cc, ss = r[m], c[m], st[m]
    order = np.lexsort((cc, ss, rr))  # by row, then strength, then column: the last of a row's run wins
    rr, cc = rr[order], cc[order]
    last = np.flatnonzero(np.r_[rr[1:] != rr[:-1], True]) if len(rr) else np.zeros(0, np.int64)
    s[rr[last]] = cc[last]
    return s


def merge_repeats(A):
    """(rows, cols, vals) with a repeated column as one entry, its values summed in stored order."""
    r, c = A.rows, A.cols
    hs = np.flatnonzero(np.r_[True, (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
    return r[hs], c[hs], seq_sums(hs, np.diff(np.r_[hs, len(c)]), A.vals)


def diagonal(A):
    ur, uc, ue = merge_repeats(A)
    d = np.zeros(A.n)
    d[ur[ur == uc]] = ue[ur == uc]
    return d


def coarsen(A):
    """(agg as coarse indices, A_c, rounds run) of one level, or None when nothing shrinks."""
    n, r, c, v = A.n, A.rows, A.cols, A.vals
    ur, uc, ue = merge_repeats(A)
    d = diagonal(A)
    key = ur * n + uc
    pos = np.minimum(np.searchsorted(key, uc * n + ur), len(key) - 1)  # the twin, 0 when the pattern has none
    twin = np.where(key[pos] == uc * n + ur, ue[pos], 0.0)
    off = ur != uc
    ur, uc = ur[off], uc[off]
    w = 0.5 * (np.abs(ue[off]) + np.abs(twin[off]))
    st = w / np.maximum(np.abs(d[ur]), np.abs(d[uc]))
    agg = np.full(n, -1, np.int64)
    prev, rounds = n, 0
    for _ in range(ROUNDS):
        rounds += 1
        s = strongest(n, ur, uc, st, agg, False)
        i = np.flatnonzero(s >= 0)
        i = i[s[s[i]] == i]
        agg[i] = np.minimum(i, s[i])
        left = int((agg == -1).sum())
        if left == 0 or left == prev or left < 0.05 * n:
            break
        prev = left
    s = strongest(n, ur, uc, st, agg, True)
    rest = np.flatnonzero(agg == -1)
    joined = np.where(s[rest] >= 0, agg[np.maximum(s[rest], 0)], rest)  # (reads the aggregation as the rounds left it)
    agg[rest] = joined
    roots = np.flatnonzero(agg == np.arange(n))
    if len(roots) == n:
        return None
    cidx = np.searchsorted(roots, agg)
    nc = len(roots)
    k = cidx[r] * nc + cidx[c]
    order = np.argsort(k, kind="stable")  # ascending (i, stored position) within every (I, J)
    ks = k[order]
    hs = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cv = seq_sums(hs, np.diff(np.r_[hs, len(ks)]), v[order])
    cr, cc = ks[hs] // nc, ks[hs] % nc
    rp = np.concatenate([[0], np.cumsum(np.bincount(cr, minlength=nc))])
    return cidx, Csr(rp, cc, cv), rounds


class Ref:
    """The hierarchy of (rowptr, cols, vals) and its V-cycle."""

    def __init__(self, oracle, rowptr, cols, vals, maxLevels=9, minCoarseRows=10, coarseSolverIters=4):
        self.oracle, self.iters = oracle, coarseSolverIters
        self.A, self.agg, self.rounds = [Csr(rowptr, cols, vals)], [], []
        while len(self.agg) < maxLevels and self.A[-1].n > minCoarseRows:
            got = coarsen(self.A[-1])
            if got is None:
                break
            self.agg.append(got[0])
            self.A.append(got[1])
            self.rounds.append(got[2])
        self.inv_d = [1.0 / diagonal(A) for A in self.A]
        self.members = []
        for agg, A in zip(self.agg, self.A[1:]):
            order = np.argsort(agg, kind="stable")
            self.members.append((order, np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=A.n))])))

    @property
    def levels(self):
        return len(self.A)

    def sweep(self, l, b, x, A=None):
        return x + OMEGA * ((b - (A or self.A[l]).mul(x)) * self.inv_d[l])

    def cg(self, A, b):
        x, r, p = np.zeros(A.n), b.copy(), np.zeros(A.n)
        rho, prev = 0.0, 1.0
        with blocked(self.oracle, capi.lib().ogl_reduction_chunk_rows()):
            for it in range(self.iters):
                prev = 1.0 if it == 0 else rho
                rho = self.oracle.dot(r, r)
                tmp = 0.0 if prev == 0.0 else rho / prev
                p = r + tmp * p
                q = A.mul(p)
                beta = self.oracle.dot(p, q)
                if beta != 0.0:
                    t = rho / beta
                    x = x + t * p
                    r = r - t * q
        return x

    def cycle(self, l, b, fine=None):
        A = fine if (l == 0 and fine is not None) else self.A[l]
        if l == self.levels - 1:
            return self.cg(A, b)
        x = OMEGA * (b * self.inv_d[l])
        x = self.sweep(l, b, x, A)
        res = b - A.mul(x)
        order, ptr = self.members[l]
        bc = seq_sums(ptr[:-1], np.diff(ptr), res[order], init=np.zeros(len(ptr) - 1))
        x = x + self.cycle(l + 1, bc)[self.agg[l]]
        x = self.sweep(l, b, x, A)
        return self.sweep(l, b, x, A)

    def apply(self, r, fine=None):
        """fine: the matrix whose products the fine level takes (a stored hierarchy applied to newer coefficients)."""
        return self.cycle(0, np.asarray(r, np.float64), fine)


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
def cfg(solver=capi.SOLVER_CG, **kw):
    base = dict(solver=solver, preconditioner=capi.PRECOND_MULTIGRID, tolerance=1e-8, rel_tol=0.0, max_iter=2000,
                renumber=capi.RENUMBER_OFF)
    base.update(kw)
    return capi.default_config(**base)


def device(reg, name, case, mg=None, props=(), **kw):
    """A solver that has solved once (ones as the right-hand side), so that its hierarchy is set up."""
    s = reg.solver(name, cfg(**kw))
    s.set_multigrid(**dict(DEFAULTS, **(mg or {})))
    for k, v in props:
        s.set_property(k, v)
    s.set_matrix(case)
    s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    return s


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


def assert_hierarchy(s, ref):
    assert s.get_property("mgLevels") == ref.levels
    total = 0
    for l, A in enumerate(ref.A):
        rp, cols, vals, agg = s.mg_level(l)
        assert s.get_property(f"mgRows{l}") == A.n and s.get_property(f"mgNnz{l}") == len(A.cols)
        np.testing.assert_array_equal(rp, A.rp, err_msg=f"row_ptrs of level {l}")
        np.testing.assert_array_equal(cols, A.cols, err_msg=f"cols of level {l}")
        np.testing.assert_array_equal(vals, A.vals, err_msg=f"vals of level {l}")
        if l + 1 < ref.levels:
            np.testing.assert_array_equal(agg, ref.agg[l], err_msg=f"agg of level {l}")
        else:
            assert agg is None
        total += len(A.cols)
    assert s.get_property("mgOperatorComplexity") == total / len(ref.A[0].cols)


CASES = {
    "poisson_sym": lambda: synthetic.poisson_case(12),
    "poisson_asym": lambda: synthetic.poisson_case(12, symmetric=False),
    "voronoi": lambda: synthetic.voronoi_case(3000),
    "long_rows": lambda: synthetic.long_rows_case(synthetic.poisson_case(14), 0.2, 14),
    "periodic_x": lambda: synthetic.poisson_block(10, 8, 6, periodic_x=True),
}
_cases, _refs = {}, {}


def ref_of(oracle, name, **mg):
    """(case, reference) of a named case, each built once."""
    if name not in _cases:
        _cases[name] = CASES[name]()
    key = (name, tuple(sorted(mg.items())))
    if key not in _refs:
        _refs[key] = Ref(oracle, *oracle_csr(oracle, _cases[name]), **dict(DEFAULTS, **mg))
    return _cases[name], _refs[key]


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _refs.clear()
    _cases.clear()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hierarchy_bit_identical(oracle, reg, name):
    case, ref = ref_of(oracle, name)
    assert ref.levels >= 3
    if name == "poisson_sym":
        assert ref.rounds[0] == 11  # (uniform weights: every strength ties, the larger column wins round after round)
    assert_hierarchy(device(reg, "h_" + name, case), ref)


# which SpMV layout stands in front: name -> (config, (spmvLayout, symmetricHalf))
LAYOUTS = {
    "half": (dict(), (2.0, 1.0)),
    "sell": (dict(symmetric_half=0), (2.0, 0.0)),
    "csr_stream": (dict(compress_indices=0), (0.0, 0.0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_apply_bit_identical(oracle, reg, name):
    """z = M^-1 r for coarseSolverIters 0, 1 and 4, and with mgTailRows at 0, between two levels and beyond the fine level."""
    r = None
    for iters in (4, 1, 0):
        case, ref = ref_of(oracle, name, coarseSolverIters=iters)
        r = rhs(case.n_cells)
        want = ref.apply(r)
        tails = (0.0, float(ref.A[2].n), float(case.n_cells + 1)) if iters == 4 else (None,)
        for tail in tails:
            s = device(reg, f"a_{name}", case, mg=dict(coarseSolverIters=iters),
                       props=() if tail is None else (("mgTailRows", tail),))
            np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{name} iters {iters} tail {tail}")
            if tail is not None:
                in_tail = sum(1 for A in ref.A if A.n <= tail)
                assert s.get_property("mgTailLevels") == in_tail and s.get_property("mgTailRows") == tail
                assert (s.get_property("mgLaunchesPerApply") == 1) == (in_tail == ref.levels)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_apply_bit_identical_on_every_layout(oracle, reg, layout):
    case, ref = ref_of(oracle, "poisson_sym")
    r = rhs(case.n_cells)
    kw, (lay, half) = LAYOUTS[layout]
    s = device(reg, "lay_" + layout, case, props=(("streamAboveBytes", 0.0),), **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))


def line_or_slab(rows):
    return synthetic.poisson_block(rows, 1, 1)


@pytest.mark.parametrize("what", ["maxLevels0", "minCoarseRows_n", "maxLevels1", "minCoarseRows1", "diagonal",
                                  "rows511", "rows512", "rows513"])
def test_hierarchy_edges(oracle, reg, what):
    mg = {}
    case = synthetic.poisson_case(12)
    levels = None
    if what == "maxLevels0":
        mg, levels = dict(maxLevels=0), 1
    elif what == "minCoarseRows_n":
        mg, levels = dict(minCoarseRows=case.n_cells), 1
    elif what == "maxLevels1":
        mg, levels = dict(maxLevels=1), 2
    elif what == "minCoarseRows1":
        mg = dict(minCoarseRows=1)
    elif what == "diagonal":  # no neighbours: every row a singleton, the coarsening is dropped
        line = synthetic.poisson_block(40, 1, 1)
        none = np.zeros(0, np.int32)
        case = synthetic.LduCase(40, none, none, line.diag, np.zeros(0), None, [], line.global_index, 40)
        levels = 1
    else:  # the chunk edge of the restriction and of the CG's reduction tree (maxLevels 0: the CG runs on these rows)
        case = line_or_slab(int(what[4:]))
    variants = [mg] if not what.startswith("rows") else [dict(), dict(maxLevels=0)]
    for variant in variants:
        ref = Ref(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, **variant))
        if levels is not None:
            assert ref.levels == levels
        if what == "minCoarseRows1":
            assert ref.A[-1].n <= 4, ref.A[-1].n
        r = rhs(case.n_cells)
        want = ref.apply(r)
        for tail in (0.0, float(case.n_cells)):  # (launch by launch, and everything in the single-workgroup tail)
            s = device(reg, f"e_{what}", case, mg=variant, props=(("mgTailRows", tail),))
            assert_hierarchy(s, ref)
            np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{variant} tail {tail}")
            assert s.get_property("mgTailLevels") == (0 if tail == 0.0 else ref.levels)


def test_renumbered_equals_caller_numbering(oracle, reg):
    """The hierarchy is that of the caller's numbering: with renumber on, z carries the same bits."""
    case = synthetic.renumber_case(synthetic.poisson_case(14), 4096)
    r = rhs(case.n_cells)
    z0 = device(reg, "rn_off", case, renumber=capi.RENUMBER_OFF).apply_preconditioner(r)
    s1 = device(reg, "rn_on", case, renumber=capi.RENUMBER_ON)
    assert s1.get_property("renumbered") == 1.0  # (the device copy really is in a numbering of its own)
    np.testing.assert_array_equal(s1.apply_preconditioner(r), z0)
    ref = Ref(oracle, *oracle_csr(oracle, case))
    assert_hierarchy(s1, ref)
    np.testing.assert_array_equal(z0, ref.apply(r))


def scaled(case, factor, rows):
    c = copy.copy(case)
    c.diag = case.diag.copy()
    c.diag[rows] *= factor
    return c


def test_values_refresh_gives_new_hierarchy(oracle, reg):
    case = synthetic.poisson_case(10)
    r = rhs(case.n_cells)
    s = device(reg, "refresh", case)
    agg_before = s.mg_level(0)[3].copy()
    case2 = scaled(case, 1.5, slice(0, case.n_cells, 3))
    s = device(reg, "refresh", case2)
    ref = Ref(oracle, *oracle_csr(oracle, case2))
    assert not np.array_equal(s.mg_level(0)[3], agg_before)  # (the aggregates really changed)
    assert_hierarchy(s, ref)
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))


def test_caching_reuses_stored_hierarchy(oracle):
    """caching 2: the second and third solve use the stored hierarchy (of the first coefficients; the fine level's products
    are those of the current matrix), the fourth generates afresh."""
    case = synthetic.poisson_case(10)
    r = rhs(case.n_cells)
    reg = capi.Registry()
    cases, refs, zs, aggs = [], [], [], []
    for step in range(4):
        cs = scaled(case, 1.0 + 0.5 * step, slice(0, case.n_cells, 3))
        cases.append(cs)
        refs.append(Ref(oracle, *oracle_csr(oracle, cs)))
        s = device(reg, "cache", cs, caching=2)
        zs.append(s.apply_preconditioner(r))
        aggs.append(s.mg_level(0)[3].copy())
    reg.close()
    for step, stored in ((0, 0), (1, 0), (2, 0), (3, 3)):
        np.testing.assert_array_equal(aggs[step], refs[stored].agg[0], err_msg=f"step {step}")
        np.testing.assert_array_equal(zs[step], refs[stored].apply(r, fine=refs[step].A[0]), err_msg=f"step {step}")
    assert not np.array_equal(refs[3].agg[0], refs[0].agg[0])


def test_mg_level_after_pattern_change_is_a_state_error(reg):
    s = device(reg, "stale", synthetic.poisson_case(8))
    s.mg_level(1)
    s = reg.solver("stale", cfg()).set_matrix(synthetic.poisson_case(9))
    with pytest.raises(capi.OglError) as e:
        s.mg_level(1)
    assert e.value.status == capi.ERR_STATE, e.value


@pytest.mark.parametrize("solver,symmetric", [(capi.SOLVER_CG, True), (capi.SOLVER_BICGSTAB, False),
                                              (capi.SOLVER_GMRES, True)])
def test_solves_converge(reg, solver, symmetric):
    case = synthetic.poisson_case(20, symmetric=symmetric)
    xs = synthetic.x_star(case.global_index, case.global_n)
    b = synthetic.apply_case(case, xs)
    out = {}
    for graph in (1.0, 0.0):
        s = reg.solver(f"solve_{solver}_{graph}", cfg(solver=solver, tolerance=1e-9))
        s.set_property("hipGraph", graph)
        s.set_matrix(case)
        x, perf = s.solve(b, np.zeros_like(b))
        assert 0 < perf.n_iterations < 2000 and perf.final_residual <= 1e-9, (perf.n_iterations, perf.final_residual)
        # the true residual, normalised as the criterion does (StoppingCriterion.H:136), meets the tolerance too
        true_res = np.abs(b - synthetic.apply_case(case, x)).sum() / perf.norm_factor
        assert true_res <= 2e-9, (true_res, perf.final_residual)
        assert np.abs(x - xs).max() < 1e-5
        out[graph] = (x, perf.n_iterations)
    assert out[1.0][1] == out[0.0][1]
    np.testing.assert_array_equal(out[1.0][0], out[0.0][0])


def test_multigrid_halves_the_iterations_of_jacobi(reg):
    case = synthetic.poisson_case(24)
    b = synthetic.apply_case(case, synthetic.x_star(case.global_index, case.global_n))
    its = {}
    for kind, pc in (("MG", capi.PRECOND_MULTIGRID), ("BJ", capi.PRECOND_BJ)):
        c = capi.default_config(solver=capi.SOLVER_CG, preconditioner=pc, tolerance=1e-6, rel_tol=0.0, max_iter=2000,
                                renumber=capi.RENUMBER_OFF)
        _, perf = reg.solver("it_" + kind, c).set_matrix(case).solve(b, np.zeros_like(b))
        its[kind] = perf.n_iterations
    assert 2 * its["MG"] < its["BJ"], its


@pytest.mark.parametrize("key,value,status", [("cycle", "w", capi.ERR_UNSUPPORTED), ("cycle", "f", capi.ERR_UNSUPPORTED),
                                              ("zeroGuess", False, capi.ERR_UNSUPPORTED),
                                              ("maxLevels", -1, capi.ERR_INVALID)])
def test_refusals(reg, key, value, status):
    case = synthetic.poisson_case(6)
    s = reg.solver(f"refuse_{key}_{value}", cfg()).set_multigrid(**{key: value}).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == status and key in str(e.value), e.value


def test_time_steps_leave_no_memory_behind():
    """20 time steps that alternate between two coefficient sets: the ledger stands still after the first four, and
    nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    sets = [case, scaled(case, 1.5, slice(0, case.n_cells, 3))]
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(20):
        s = reg.solver("steps", cfg()).set_matrix(sets[step % 2])
        s.solve(b, np.zeros_like(b))
        if step in (3, 19):
            marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[19][k] == marks[3][k], (k, marks)
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
