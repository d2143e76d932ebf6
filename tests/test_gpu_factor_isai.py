"""Keywords triangularSolves isai and factorSweeps N of IC / ILU / IRILU (kernels_factor.hip: k_factor_isai_generate,
k_factor_sweep_start, k_factor_sweep) through the C ABI against the walk of the contract
(tests/factor_isai_walk.py): z = M^-1 r bit for bit, whole solves bit for bit with the oracle's Krylov loop calling the
walk back as its preconditioner, the same bits on every layout and numbering, the refusals, the breakdown, time steps with
caching, and two ranks (tests/factor_isai_worker.py)."""
import copy
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import oracle_csr
import factor_isai_walk as fw
import precond_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"IC": capi.PRECOND_IC, "ILU": capi.PRECOND_ILU, "IRILU": capi.PRECOND_IRILU}
ASYM = dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
BOXES = {"b666": (6, 6, 6),      # 216 rows: one chunk
         "b1097": (10, 9, 7),    # 630 rows: a partial second chunk
         "b997": (9, 9, 7),      # 567 rows, odd
         "b13911": (13, 9, 11)}  # 1,287 rows
# (IC on the random system reads its lower triangle alone: the apply is pinned there too -- the update lists of IC's sweeps
#  are not trivial on a graph with triangles --, no solve is judged)
SYSTEMS = [(name, kind) for name in BOXES for kind in ("IC", "ILU")] + [("random", "ILU"), ("random", "IC")]


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def system(name, kind):
    """(case, b, (rowptr, cols, vals)): boxes symmetric for IC and asymmetric for ILU / IRILU; the random system."""
    if name == "random":
        case = fw.random_system()
        b = np.random.default_rng(5).uniform(-1, 1, case.n_cells)
    else:
        case = synthetic.poisson_block(*BOXES[name], **({} if kind == "IC" else ASYM))
        b = synthetic.rhs_for_x_star(case)[0]
    return case, b, oracle_csr(_oracle(), case)


@functools.lru_cache(maxsize=None)
def walk(name, kind, isai, power, sweeps):
    """Computed once per process; do not change it."""
    return fw.Walk(_oracle(), *system(name, "IC" if kind == "IC" else "ILU")[2], kind, isai=isai, power=power, sweeps=sweeps)


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


def make(reg, field, kind, isai=None, power=1, sweeps=None, solver=None, **kw):
    solver = solver if solver is not None else (capi.SOLVER_CG if kind == "IC" else capi.SOLVER_BICGSTAB)
    base = dict(solver=solver, preconditioner=KINDS[kind], sparsity_power=power, tolerance=1e-9, rel_tol=0.0, max_iter=300,
                export_res=1, adapt_min_iter=0, update_init_guess=1, renumber=capi.RENUMBER_OFF)
    base.update(kw)
    s = reg.solver(field, capi.default_config(**base))
    if isai is not None:
        s.set_triangular_solves("isai" if isai else "exact")
    if sweeps is not None:
        s.set_factor_sweeps(sweeps)
    return s


def solve(s, case, b):
    s.set_matrix(case)
    return s.solve(b, np.zeros_like(b))


@pytest.fixture
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.mark.parametrize("name,kind", SYSTEMS, ids=lambda v: str(v))
def test_apply_bits(reg, name, kind):
    case, b, _ = system(name, kind)
    r = rhs(case.n_cells)
    few = dict(max_iter=3) if (name, kind) == ("random", "IC") else {}  # (CG on an asymmetric matrix: only z is looked at)
    for power in (1, 2):
        for sweeps in (0, 1, 3):
            s = make(reg, f"{name}_{kind}", kind, True, power, sweeps, **few)
            solve(s, case, b)
            w = walk(name, kind, True, power, sweeps)
            np.testing.assert_array_equal(s.apply_preconditioner(r), w.apply(r), err_msg=f"p {power} sweeps {sweeps}")
            assert s.get_property("triangularSolvesInUse") == 1.0 and s.get_property("factorSweepsInUse") == sweeps
            assert s.get_property("triangularWEntries") == w.w_entries
            assert s.get_property("iluLaunchesPerApply") == 2.0 and s.get_property("iluBreakdownRow") == -1.0
    # the swept factor under the exact solves, and under IRILU's sweeps
    for k in (kind, "IRILU") if kind == "ILU" else (kind,):
        s = make(reg, f"{name}_{k}_exact", k, False, 1, 3, **few)
        solve(s, case, b)
        np.testing.assert_array_equal(s.apply_preconditioner(r), walk(name, k, False, 1, 3).apply(r), err_msg=k)
        assert s.get_property("triangularSolvesInUse") == 0.0 and s.get_property("factorSweepsInUse") == 3.0


def assert_is_the_oracles(s, x, perf, ref, bicgstab):
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)
    assert perf.n_iterations == (ref.n_iterations // 2 if bicgstab else ref.n_iterations)
    assert perf.n_norm_evals == ref.n_evals
    assert perf.initial_residual == ref.initial_residual and perf.final_residual == ref.final_residual
    assert perf.norm_factor == ref.norm_factor


@pytest.mark.parametrize("power,sweeps", [(1, 0), (2, 3)])
@pytest.mark.parametrize("name,kind", [(n, "IC") for n in BOXES] + [("random", "ILU")], ids=lambda v: str(v))
def test_whole_solves(reg, name, kind, power, sweeps):
    oracle = _oracle()
    case, b, csr = system(name, kind)
    s = make(reg, f"solve_{name}", kind, True, power, sweeps)
    x, perf = solve(s, case, b)
    solver = "cg" if kind == "IC" else "bicgstab"
    ref = pc.oracle_solve(oracle.DistMatrix(*csr), b, pc.callback(walk(name, kind, True, power, sweeps).apply), solver)
    assert ref.final_residual <= pc.TOL and ref.n_iterations >= 5, (ref.n_iterations, ref.final_residual)
    assert_is_the_oracles(s, x, perf, ref, solver == "bicgstab")


@pytest.mark.parametrize("name,kind", [("b13911", "IC"), ("b1097", "ILU"), ("random", "ILU")], ids=lambda v: str(v))
def test_same_bits_on_every_layout_and_numbering(reg, name, kind):
    case, b, _ = system(name, kind)
    if name != "random":  # (what `renumber` on reorders)
        case = synthetic.renumber_case(case, 4096)
        want = fw.Walk(_oracle(), *oracle_csr(_oracle(), case), kind, power=2, sweeps=1)
    else:
        want = walk(name, kind, True, 2, 1)
    b = np.ones(case.n_cells)
    r = rhs(case.n_cells)
    seen = set()
    for compress in (0, 1):
        for renumber in (capi.RENUMBER_OFF, capi.RENUMBER_ON):
            s = make(reg, f"lay_{compress}_{renumber}", kind, True, 2, 1, compress_indices=compress, renumber=renumber)
            solve(s, case, b)
            seen.add((compress, s.get_property("renumbered")))
            np.testing.assert_array_equal(s.apply_preconditioner(r), want.apply(r), err_msg=f"{compress} {renumber}")
            assert s.get_property("iluLaunchesPerApply") == (4.0 if s.get_property("renumbered") else 2.0)
    if name != "random":
        assert (0, 1.0) in seen and (1, 1.0) in seen  # (the device copy really was in a numbering of its own)


@pytest.mark.parametrize("kind", ["IC", "ILU"])
def test_defaults_are_exact_and_zero(reg, kind):
    case, b, csr = system("b997", kind)
    r = rhs(case.n_cells)
    s = make(reg, "defaults", kind)
    solve(s, case, b)
    z = s.apply_preconditioner(r)
    assert s.get_property("triangularSolvesInUse") == 0.0 and s.get_property("factorSweepsInUse") == 0.0
    s = make(reg, "defaults", kind, False, 1, 0)
    solve(s, case, b)
    np.testing.assert_array_equal(s.apply_preconditioner(r), z)
    np.testing.assert_array_equal(z, walk("b997", kind, False, 1, 0).apply(r))


def test_refusals(reg):
    case, b, _ = system("b666", "IC")
    s = make(reg, "refuse", "IC")
    for key, bad in (("triangularSolves", 2.0), ("triangularSolves", 0.5), ("factorSweeps", 11.0), ("factorSweeps", -1.0),
                     ("factorSweeps", 2.5)):
        s.set_property(key, bad)
        with pytest.raises(capi.OglError) as e:
            solve(s, case, b)
        assert e.value.status == capi.ERR_INVALID and key in str(e.value), e.value
        s.set_property(key, 0.0)
        _, perf = solve(s, case, b)  # the same handle solves
        assert perf.final_residual <= 1e-9
    # every other preconditioner ignores the keywords
    s = make(reg, "bj", "IC", preconditioner=capi.PRECOND_BJ)
    s.set_property("triangularSolves", 7.0)
    assert solve(s, case, b)[1].final_residual <= 1e-9
    # IRILU + isai
    case, b, _ = system("b666", "ILU")
    s = make(reg, "irilu", "IRILU", True)
    with pytest.raises(capi.OglError) as e:
        solve(s, case, b)
    assert e.value.status == capi.ERR_UNSUPPORTED and "IRILU" in str(e.value) and "isai" in str(e.value), e.value
    s.set_triangular_solves("exact")
    assert solve(s, case, b)[1].final_residual <= 1e-9


def test_a_wide_row_of_w_is_refused(reg):
    case = fw.random_system(hub=12)
    csr = oracle_csr(_oracle(), case)
    rp, c, _, diag = fw.factor_pattern(*[np.asarray(x) for x in csr], False)
    widths = [max(len(r) for r in fw.w_pattern(rp, c, diag, p)) for p in (1, 2)]
    assert widths[0] <= fw.MAX_W_ROW < widths[1], widths
    wide = next(i for i, r in enumerate(fw.w_pattern(rp, c, diag, 2)) if len(r) > fw.MAX_W_ROW)
    b = np.ones(case.n_cells)
    s = make(reg, "hub", "ILU", True, 2)
    with pytest.raises(capi.OglError) as e:
        solve(s, case, b)
    msg = str(e.value)
    assert e.value.status == capi.ERR_UNSUPPORTED and "ILU" in msg and f"row {wide} " in msg and "lower sparsityPower" in msg
    s = make(reg, "hub", "ILU", True, 1)  # the same handle solves on, at p = 1
    solve(s, case, b)
    r = rhs(case.n_cells)
    np.testing.assert_array_equal(s.apply_preconditioner(r), fw.Walk(_oracle(), *csr, "ILU", power=1).apply(r))


def test_breakdown_after_the_last_sweep(reg):
    case = copy.copy(system("b666", "IC")[0])
    case.diag = case.diag.copy()
    case.diag[5] = -case.diag[5]
    w = fw.Walk(_oracle(), *oracle_csr(_oracle(), case), "IC", isai=False, sweeps=3)
    assert w.breakdown == 5
    for isai in (False, True):
        s = make(reg, f"neg{isai}", "IC", isai, 1, 3)
        with pytest.raises(capi.OglError) as e:
            solve(s, case, np.ones(case.n_cells))
        assert e.value.status == capi.ERR_INVALID and "IC" in str(e.value) and "non-positive pivot in row 5 " in str(e.value)
        assert s.get_property("iluBreakdownRow") == 5.0


@pytest.mark.parametrize("caching", [0, 3])
def test_time_steps_and_caching(reg, caching):
    """Coefficients changed per step: with caching N the stored object (step 0's) serves N solves, then one solve generates
    for itself (Preconditioner.H:353-431) -- each z is the walk's of the matrix its object was generated from."""
    import soak_worker
    base = system("b1097", "IC")[0]
    r = rhs(base.n_cells)
    b = np.ones(base.n_cells)
    marks, first = {}, None
    for step in range(10):
        case = copy.copy(base)
        case.diag = base.diag * (1.0 + 0.125 * step)
        s = make(reg, "steps", "IC", True, 2, 2, caching=caching)
        solve(s, case, b)
        own = step % (caching + 1) == 0
        if step == 0 or own:
            w = fw.Walk(_oracle(), *oracle_csr(_oracle(), case), "IC", power=2, sweeps=2)
            first = first or w
        np.testing.assert_array_equal(s.apply_preconditioner(r), (w if own else first).apply(r), err_msg=f"step {step}")
        if step in (4, 9):
            marks[step] = capi.memory_ledger().as_dict()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[9][k] - marks[4][k] == 0, (k, marks)


def test_switching_between_solves_regenerates(reg):
    case, b, _ = system("b997", "ILU")
    r = rhs(case.n_cells)
    for isai, power, sweeps in ((True, 1, 0), (False, 1, 0), (True, 2, 3), (True, 2, 0), (False, 1, 3), (True, 1, 0)):
        s = make(reg, "switch", "ILU", isai, power, sweeps)
        solve(s, case, b)
        assert s.get_property("triangularSolvesInUse") == float(isai) and s.get_property("factorSweepsInUse") == sweeps
        np.testing.assert_array_equal(s.apply_preconditioner(r), walk("b997", "ILU", isai, power, sweeps).apply(r),
                                      err_msg=f"{isai} {power} {sweeps}")
    # back on exact / 0 the buffers of W and of the sweeps are released: the ledger is where an exact-only handle leaves it
    s = make(reg, "switch", "ILU", False, 1, 0)
    solve(s, case, b)
    after = capi.memory_ledger().as_dict()["device_bytes"]
    s = make(reg, "switch", "ILU", True, 2, 3)
    solve(s, case, b)
    assert capi.memory_ledger().as_dict()["device_bytes"] > after
    s = make(reg, "switch", "ILU", False, 1, 0)
    solve(s, case, b)
    assert capi.memory_ledger().as_dict()["device_bytes"] == after


def test_a_stored_object_is_applied_the_way_it_was_generated(reg):
    case, b, _ = system("b997", "IC")
    r = rhs(case.n_cells)
    a = make(reg, "field_a", "IC", True, 2, 1, caching=2)
    solve(a, case, b)
    other = make(reg, "field_b", "IC", False, 1, 0, caching=2)  # asks for exact / 0 ...
    other.set_property("preconditionerCaching", 2.0)            # ... and adopts the stored object
    solve(other, case, b)
    assert other.get_property("preconditionerCaching") == 1.0
    assert other.get_property("triangularSolvesInUse") == 1.0 and other.get_property("factorSweepsInUse") == 1.0
    np.testing.assert_array_equal(other.apply_preconditioner(r), walk("b997", "IC", True, 2, 1).apply(r))


def test_two_ranks():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "factor_isai_worker.py")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count(" ok") == 2, p.stdout
