"""Preconditioner Multigrid with `aggregation hashed` and `aggregatePasses p` ("hashed ties" and
"passes") against a NumPy restatement of that contract: `coarsen` with the tie rule as an argument and `PassRef`, the
reference of tests/test_gpu_multigrid.py with the pass loop -- its V-cycle, sums and coarsest CG are that file's own,
imported unchanged.  Aggregates integer-exact, coarse matrices and z = M^-1 r bit for bit, whole solves against the oracle's
loop in the device's reduction tree with the reference called back as its preconditioner (tests/precond_cases.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ogl_amd import capi, synthetic  # noqa: E402
from helpers import oracle_csr  # noqa: E402
import precond_cases as pc  # noqa: E402
import test_gpu_multigrid as base  # noqa: E402
import test_gpu_precond_solves as solves  # noqa: E402
from test_gpu_multigrid import Csr, Ref, diagonal, merge_repeats, seq_sums  # noqa: E402

pytestmark = pytest.mark.gpu

ROUNDS = base.ROUNDS
DEFAULTS = base.DEFAULTS
VARIANTS = [("hashed", 1), ("hashed", 3), ("pgm", 2)]


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def edge_hash(i, j):
    """h(min(i, j), max(i, j)) in unsigned 32-bit wrap-around arithmetic."""
    a, b = np.minimum(i, j).astype(np.uint32), np.maximum(i, j).astype(np.uint32)
    h = (a * np.uint32(0x9E3779B1)) ^ (b * np.uint32(0x85EBCA6B) + np.uint32(0xC2B2AE35))
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    return h


def strongest(n, r, c, st, tie, agg, want_aggregated):
    """s[i] for the unaggregated rows i: the neighbour (aggregated or not, as asked) of the largest (strength, tie, column);
    -1: none."""
    s = np.full(n, -1, np.int64)
    m = (agg[r] == -1) & ((agg[c] != -1) == want_aggregated)
    rr, cc, ss, tt = r[m], c[m], st[m], tie[m]
    order = np.lexsort((cc, tt, ss, rr))  # by row, strength, tie, column: the last of a row's run wins
    rr, cc = rr[order], cc[order]
    last = np.flatnonzero(np.r_[rr[1:] != rr[:-1], True]) if len(rr) else np.zeros(0, np.int64)
    s[rr[last]] = cc[last]
    return s


def coarsen(A, aggregation):
    """(agg as coarse indices, A_c, rounds run) of one pairwise coarsening (rules 1-5), or None when nothing shrinks.
    aggregation 'pgm': equal strengths go to the larger column; 'hashed': to the larger edge hash first."""
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
    tie = edge_hash(ur, uc) if aggregation == "hashed" else np.zeros(len(ur), np.uint32)
    agg = np.full(n, -1, np.int64)
    prev, rounds = n, 0
    for _ in range(ROUNDS):
        rounds += 1
        s = strongest(n, ur, uc, st, tie, agg, False)
        i = np.flatnonzero(s >= 0)
        i = i[s[s[i]] == i]
        agg[i] = np.minimum(i, s[i])
        left = int((agg == -1).sum())
        if left == 0 or left == prev or left < 0.05 * n:
            break
        prev = left
    s = strongest(n, ur, uc, st, tie, agg, True)
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


class PassRef(Ref):
    """The hierarchy whose kept levels are made of up to aggregatePasses coarsenings each; agg: the composite maps,
    passes[l]: how many made level l + 1.  The V-cycle is Ref's."""

    def __init__(self, oracle, rowptr, cols, vals, maxLevels=9, minCoarseRows=10, coarseSolverIters=4, aggregation="pgm",
                 aggregatePasses=1):
        self.oracle, self.iters = oracle, coarseSolverIters
        self.A, self.agg, self.rounds, self.passes = [Csr(rowptr, cols, vals)], [], [], []
        while len(self.agg) < maxLevels and self.A[-1].n > minCoarseRows:
            A, comp, rounds = self.A[-1], None, []
            for _ in range(aggregatePasses):
                got = coarsen(A, aggregation)
                if got is None:  # (dropped: it ends the level's passes)
                    break
                comp = got[0] if comp is None else got[0][comp]
                A = got[1]
                rounds.append(got[2])
                if A.n <= minCoarseRows:
                    break
            if comp is None:
                break
            self.agg.append(comp)
            self.A.append(A)
            self.rounds.append(rounds)
            self.passes.append(len(rounds))
        self.inv_d = [1.0 / diagonal(A) for A in self.A]
        self.members = []
        for agg, A in zip(self.agg, self.A[1:]):
            order = np.argsort(agg, kind="stable")
            self.members.append((order, np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=A.n))])))


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
def mg_of(aggregation, passes, **mg):
    return dict(mg, aggregation=aggregation, aggregatePasses=passes)


def device(reg, name, case, aggregation, passes, mg=None, props=(), **kw):
    return base.device(reg, name, case, mg=mg_of(aggregation, passes, **(mg or {})), props=props, **kw)


def assert_hierarchy(s, ref):
    base.assert_hierarchy(s, ref)
    for l, p in enumerate(ref.passes):
        assert s.get_property(f"mgPasses{l}") == p, (l, ref.passes)


_cases, _refs = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = base.CASES[name]()
    return _cases[name]


def ref_of(oracle, name, aggregation, passes, **mg):
    """(case, reference) of a named case, each built once."""
    key = (name, aggregation, passes, tuple(sorted(mg.items())))
    if key not in _refs:
        _refs[key] = PassRef(oracle, *oracle_csr(oracle, case_of(name)),
                             **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes, **mg))
    return case_of(name), _refs[key]


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _refs.clear()
    _cases.clear()


@pytest.fixture(scope="module")
def ref20(oracle):
    """poisson_case(20): the case, its matrix and the references of hashed / 1 and hashed / 3."""
    case = synthetic.poisson_case(20)
    csr = oracle_csr(oracle, case)
    return case, {p: PassRef(oracle, *csr, **dict(DEFAULTS, aggregation="hashed", aggregatePasses=p)) for p in (1, 3)}


# ---- 1. the hierarchy ----
@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_hierarchy_bit_identical(oracle, reg, name, aggregation, passes):
    case, ref = ref_of(oracle, name, aggregation, passes)
    if passes < 3:
        assert ref.levels >= 3
    assert ref.levels >= 2 and max(ref.passes) == passes
    if (name, aggregation, passes) == ("poisson_sym", "hashed", 3):
        # (a level that ends before its third pass because minCoarseRows was reached)
        assert ref.passes[-1] < 3 and ref.A[-1].n <= DEFAULTS["minCoarseRows"], (ref.passes, [A.n for A in ref.A])
    assert_hierarchy(device(reg, f"h_{name}", case, aggregation, passes), ref)


# ---- 2. the apply ----
@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("name", sorted(base.CASES))
def test_apply_bit_identical(oracle, reg, name, aggregation, passes):
    """z = M^-1 r for coarseSolverIters 4 and 0, and with mgTailRows at 0, between two levels and beyond the fine level."""
    for iters in (4, 0):
        case, ref = ref_of(oracle, name, aggregation, passes, coarseSolverIters=iters)
        assert ref.levels >= 2
        r = base.rhs(case.n_cells)
        want = ref.apply(r)
        between = float(ref.A[max(1, ref.levels - 2)].n)  # (the levels from that one down in the tail, level 0 not)
        for tail in ((0.0, between, float(case.n_cells + 1)) if iters == 4 else (None,)):
            s = device(reg, f"a_{name}", case, aggregation, passes, mg=dict(coarseSolverIters=iters),
                       props=() if tail is None else (("mgTailRows", tail),))
            np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{name} iters {iters} tail {tail}")
            if tail is not None:
                in_tail = sum(1 for A in ref.A if A.n <= tail)
                assert s.get_property("mgTailLevels") == in_tail and s.get_property("mgTailRows") == tail
                assert (s.get_property("mgLaunchesPerApply") == 1) == (in_tail == ref.levels)
                if tail == between:
                    assert 0 < in_tail < ref.levels


@pytest.mark.parametrize("aggregation,passes", VARIANTS)
@pytest.mark.parametrize("layout", sorted(base.LAYOUTS))
def test_apply_bit_identical_on_every_layout(oracle, reg, layout, aggregation, passes):
    case, ref = ref_of(oracle, "poisson_sym", aggregation, passes)
    r = base.rhs(case.n_cells)
    kw, (lay, half) = base.LAYOUTS[layout]
    s = device(reg, "lay_" + layout, case, aggregation, passes, props=(("streamAboveBytes", 0.0),), **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    np.testing.assert_array_equal(s.apply_preconditioner(r), ref.apply(r))


# ---- 3. the stall ----
def test_the_stall_is_gone(oracle, reg, ref20):
    """20^3 (8,000 rows): the present contract pairs one layer per round and keeps over 0.6 n rows; hashed ties pair a fixed
    fraction per round.  The caps are those of the contract's walk (5,156; 3,516; 794), not of the device."""
    case, refs = ref20
    n = case.n_cells
    s = base.device(reg, "stall_pgm", case)
    assert s.get_property("mgRows1") > 0.6 * n, s.get_property("mgRows1")
    s = device(reg, "stall_h1", case, "hashed", 1)
    print("hashed / 1: mgRows1", s.get_property("mgRows1"))
    assert s.get_property("mgRows1") <= 0.55 * n, s.get_property("mgRows1")
    s = device(reg, "stall_h3", case, "hashed", 3)
    print("hashed / 3: mgRows1", s.get_property("mgRows1"), "rows", [A.n for A in refs[3].A])
    assert s.get_property("mgRows1") <= n / 6, s.get_property("mgRows1")
    assert_hierarchy(s, refs[3])


# ---- 4. the defaults ----
def test_defaults_are_pgm_and_one_pass(oracle, reg):
    case = case_of("poisson_sym")
    plain = base.device(reg, "def_plain", case)
    named = device(reg, "def_named", case, "pgm", 1)
    assert plain.get_property("mgLevels") == named.get_property("mgLevels") >= 3
    for l in range(int(plain.get_property("mgLevels"))):
        for a, b in zip(plain.mg_level(l), named.mg_level(l)):
            assert (a is None and b is None) or np.array_equal(a, b), l
    # (and the reference of this file at pgm / 1 is that of test_gpu_multigrid.py)
    old = Ref(oracle, *oracle_csr(oracle, case), **DEFAULTS)
    new = ref_of(oracle, "poisson_sym", "pgm", 1)[1]
    assert new.passes == [1] * (old.levels - 1) and [r[0] for r in new.rounds] == old.rounds
    assert_hierarchy(named, new)
    base.assert_hierarchy(named, old)


# ---- 5. whole solves ----
@pytest.mark.parametrize("name,solver,aggregation,passes,renumber", [
    ("sym", "cg", "hashed", 3, capi.RENUMBER_OFF), ("asym", "bicgstab", "hashed", 2, capi.RENUMBER_OFF),
    ("shuffled14", "cg", "hashed", 3, capi.RENUMBER_ON)], ids=lambda v: str(v))
def test_whole_solves_are_the_oracles(oracle, reg, name, solver, aggregation, passes, renumber):
    props = (("aggregation", float(capi.MG_AGGREGATION[aggregation])), ("aggregatePasses", float(passes)))
    got = solves.device_solve(reg, f"ws_{name}_{solver}", name, "MG", solver, props=props, renumber=renumber)
    s = got[0]
    new_id = None
    if renumber == capi.RENUMBER_ON:
        new_id = s.renumbering()
        assert new_id is not None and s.get_property("renumbered") == 1.0
        assert not np.array_equal(new_id, np.arange(new_id.size))
    key = ("whole", name, aggregation, passes)
    if key not in _refs:
        _refs[key] = PassRef(oracle, *pc.system(name)[3], **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=passes))
    assert s.get_property("mgPasses0") == _refs[key].passes[0] == passes
    ref = pc.reference(name, "MG", solver, new_id=new_id, apply=_refs[key].apply)
    pc.check_sound(ref, pc.system(name)[2], bicgstab=solver == "bicgstab")
    solves.assert_is_the_oracles(got, ref, solver)


# ---- 6. it preconditions ----
def test_hashed_three_passes_halve_the_iterations_of_jacobi(reg):
    case = synthetic.poisson_case(20)
    b = synthetic.apply_case(case, synthetic.x_star(case.global_index, case.global_n))
    its = {}
    for kind, pre in (("MG", capi.PRECOND_MULTIGRID), ("BJ", capi.PRECOND_BJ)):
        c = capi.default_config(solver=capi.SOLVER_CG, preconditioner=pre, tolerance=1e-6, rel_tol=0.0, max_iter=2000,
                                renumber=capi.RENUMBER_OFF)
        s = reg.solver("it3_" + kind, c)
        if kind == "MG":
            s.set_multigrid(aggregation="hashed", aggregatePasses=3)
        _, perf = s.set_matrix(case).solve(b, np.zeros_like(b))
        its[kind] = perf.n_iterations
    print("iterations", its)
    assert 2 * its["MG"] <= its["BJ"], its


# ---- 7. refusals and edges ----
@pytest.mark.parametrize("key,value", [("aggregatePasses", 0), ("aggregatePasses", 5), ("aggregation", 2)])
def test_refusals(reg, key, value):
    case = synthetic.poisson_case(6)
    s = reg.solver(f"agg_refuse_{key}_{value}", base.cfg()).set_multigrid(**{key: value}).set_matrix(case)
    with pytest.raises(capi.OglError) as e:
        s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    assert e.value.status == capi.ERR_INVALID and key in str(e.value), e.value


def test_an_unknown_word_is_refused_at_the_boundary(reg):
    with pytest.raises(KeyError):
        reg.solver("agg_word", base.cfg()).set_multigrid(aggregation="greedy")


@pytest.mark.parametrize("what", ["diagonal", "two_rows", "maxLevels1"])
def test_hierarchy_edges(oracle, reg, what):
    mg = {}
    if what == "diagonal":  # no neighbours: every row a singleton, the first pass is dropped and ends the hierarchy
        line = synthetic.poisson_block(40, 1, 1)
        none = np.zeros(0, np.int32)
        case = synthetic.LduCase(40, none, none, line.diag, np.zeros(0), None, [], line.global_index, 40)
        levels, passes = 1, []
    elif what == "two_rows":  # one pair; the second pass has one row left and nothing to shrink
        case, mg = synthetic.poisson_block(2, 1, 1), dict(minCoarseRows=0)
        levels, passes = 2, [1]
    else:
        case, mg = synthetic.poisson_case(12), dict(maxLevels=1)
        levels, passes = 2, [3]
    for aggregation in ("hashed", "pgm"):
        ref = PassRef(oracle, *oracle_csr(oracle, case), **dict(DEFAULTS, aggregation=aggregation, aggregatePasses=3, **mg))
        assert ref.levels == levels and ref.passes == passes, (ref.levels, ref.passes)
        r = base.rhs(case.n_cells)
        want = ref.apply(r)
        for tail in (0.0, float(case.n_cells)):
            s = device(reg, f"ae_{what}", case, aggregation, 3, mg=mg, props=(("mgTailRows", tail),))
            assert_hierarchy(s, ref)
            np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{aggregation} tail {tail}")


# ---- 8. the stored hierarchy and memory ----
def test_caching_reuses_stored_hierarchy(oracle):
    """caching 3 with hashed / 3: the second to fourth solve use the stored hierarchy (of the first coefficients; the fine
    level's products are those of the current matrix), the fifth generates afresh."""
    case = synthetic.poisson_case(10)
    r = base.rhs(case.n_cells)
    reg = capi.Registry()
    refs, zs, aggs = [], [], []
    for step in range(5):
        cs = base.scaled(case, 1.0 + 0.5 * step, slice(0, case.n_cells, 3))
        refs.append(PassRef(oracle, *oracle_csr(oracle, cs), **dict(DEFAULTS, aggregation="hashed", aggregatePasses=3)))
        s = device(reg, "agg_cache", cs, "hashed", 3, caching=3)
        zs.append(s.apply_preconditioner(r))
        aggs.append(s.mg_level(0)[3].copy())
    reg.close()
    assert refs[0].passes[0] == 3
    for step, stored in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 4)):
        np.testing.assert_array_equal(aggs[step], refs[stored].agg[0], err_msg=f"step {step}")
        np.testing.assert_array_equal(zs[step], refs[stored].apply(r, fine=refs[step].A[0]), err_msg=f"step {step}")
    assert not np.array_equal(refs[4].agg[0], refs[0].agg[0])


def test_time_steps_leave_no_memory_behind():
    """20 time steps with hashed / 3 that alternate between two coefficient sets: the ledger stands still after the first
    four, and nothing is left after close."""
    import soak_worker
    case = synthetic.poisson_case(16)
    sets = [case, base.scaled(case, 1.5, slice(0, case.n_cells, 3))]
    b = np.ones(case.n_cells)
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(20):
        s = reg.solver("agg_steps", base.cfg()).set_multigrid(aggregation="hashed", aggregatePasses=3)
        s.set_matrix(sets[step % 2]).solve(b, np.zeros_like(b))
        if step == 0:
            assert s.get_property("mgPasses0") == 3
        if step in (3, 19):
            marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[19][k] == marks[3][k], (k, marks)
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]
