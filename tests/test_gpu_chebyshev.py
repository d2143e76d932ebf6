"""Preconditioner Chebyshev (kernels_cheb.hip, solver_precond.cpp) through the C ABI against the walk
of the contract (tests/chebyshev_walk.py, pinned by tests/test_chebyshev_walk.py): (a) the generation -- the bounds bit
for bit, a forced bound, the refusals, the breakdown; (b) z = M^-1 r bit for bit, fused and unfused, on every layout and
numbering; (c) whole solves bit for bit with the oracle's loops calling the walk back, caching, the ledger; (d) two ranks
(tests/chebyshev_ranks_worker.py).  Without the feature every test fails at capi.PRECOND_CHEBYSHEV."""
import copy
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, to_new
import chebyshev_walk as cw
import gmres_ortho_walk as gw
import soak_worker
from test_gpu_guess_projection import random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOXES = {"6x6x6": (6, 6, 6),        # 216 rows: one chunk
         "10x9x7": (10, 9, 7),      # 630 rows: a partial second chunk
         "9x9x7": (9, 9, 7),        # 567 rows, odd: the one-row tail of the last pair; line length 9: not FAST
         "12x12x12": (12, 12, 12)}  # 1,728 rows: four chunks, FAST
CSR = dict(symmetric_half=0, compress_indices=0)
# name -> (system, config keywords, the in-loop layout is the whole-matrix half storage)
LAYOUTS = {**{name: (name, {}, True) for name in BOXES},
           "random": ("random", {}, False),
           "12x12x12-csr": ("12x12x12", CSR, False),
           "12x12x12-renumbered": ("12x12x12", dict(renumber=capi.RENUMBER_ON), False)}
DEGREES = (1, 2, 3, 4, 16)  # both parities of the buffer assignment, the default, the full table
TOL = 1e-8


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


@functools.lru_cache(maxsize=None)
def system(name):
    """(case, b, (rowptr, cols, vals)); built once and left unchanged."""
    case = random_case() if name == "random" else synthetic.poisson_block(*BOXES[name])
    b = np.random.default_rng(7).uniform(-1, 1, case.n_cells) if name == "random" else synthetic.rhs_for_x_star(case)[0]
    return case, b, oracle_csr(_oracle(), case)


@functools.lru_cache(maxsize=None)
def walk(name, degree=cw.DEFAULT_DEGREE, ratio=cw.DEFAULT_RATIO, lambda_max=0.0, perm=None):
    """Computed once per process; do not change it.  perm: the walk on the system permuted by that numbering."""
    rp, cols, vals = system(name)[2]
    if perm is not None:
        rp, cols, vals, _ = _oracle().permute_csr(rp, cols, vals, np.frombuffer(perm, np.int32))
    return cw.Walk(_oracle(), rp, cols, vals, degree=degree, ratio=ratio, lambda_max=lambda_max)


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)


def make(reg, field, name, degree=None, fused=None, solver=None, **kw):
    solver = solver if solver is not None else (capi.SOLVER_BICGSTAB if name == "random" else capi.SOLVER_CG)
    base = dict(solver=solver, preconditioner=capi.PRECOND_CHEBYSHEV, tolerance=TOL, rel_tol=0.0, max_iter=300, export_res=1,
                adapt_min_iter=0, update_init_guess=1, renumber=capi.RENUMBER_OFF)
    base.update(kw)
    s = reg.solver(field, capi.default_config(**base))
    s.set_chebyshev(degree=degree)
    if fused is not None:
        s.set_property("chebyshevFused", float(fused))
    return s


def solve(s, case, b):
    s.set_matrix(case)
    return s.solve(b, np.zeros_like(b))


def walk_of(s, name, **kw):
    """(the walk in the numbering of s's device copy, z(r) in the caller's order)"""
    new_id = s.renumbering()
    if new_id is None:
        w = walk(name, **kw)
        return w, w.apply
    w = walk(name, perm=np.ascontiguousarray(new_id, np.int32).tobytes(), **kw)
    return w, lambda r: w.apply(to_new(r, new_id))[new_id]


@pytest.fixture
def reg():
    r = capi.Registry()
    yield r
    r.close()


# ---------------------------------------------------------------- (a) the generation

@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_bounds_are_the_walks(reg, layout):
    name, kw, _ = LAYOUTS[layout]
    case, b, _ = system(name)
    s = make(reg, "gen", name, **kw)
    solve(s, case, b)
    w, _ = walk_of(s, name)
    print(layout, "lambda_max", w.table.lambda_max, "lambda_min", w.table.lambda_min)
    assert s.get_property("chebyshevLambdaMaxInUse") == w.table.lambda_max
    assert s.get_property("chebyshevLambdaMinInUse") == w.table.lambda_min
    # a forced bound is taken, with another ratio
    s.set_chebyshev(eig_ratio=7.5, lambda_max=1.625)
    solve(s, case, b)
    assert s.get_property("chebyshevLambdaMaxInUse") == 1.625
    assert s.get_property("chebyshevLambdaMinInUse") == cw.coefficients(1.625, 7.5).lambda_min
    _, apply = walk_of(s, name, ratio=7.5, lambda_max=1.625)
    r = rhs(case.n_cells)
    np.testing.assert_array_equal(s.apply_preconditioner(r), apply(r))


def test_refusals(reg):
    case, b, _ = system("6x6x6")
    s = make(reg, "refuse", "6x6x6")
    for key, bad, good in (("chebyshevDegree", 0.0, 4.0), ("chebyshevDegree", 17.0, 4.0), ("chebyshevDegree", 1.5, 4.0),
                           ("chebyshevEigRatio", 1.0, 30.0), ("chebyshevEigRatio", 1e6, 30.0),
                           ("chebyshevLambdaMax", -1.0, 0.0), ("chebyshevLambdaMax", float("nan"), 0.0)):
        s.set_property(key, bad)
        with pytest.raises(capi.OglError) as e:
            solve(s, case, b)
        assert e.value.status == capi.ERR_INVALID and key in str(e.value), e.value
        s.set_property(key, good)
        _, perf = solve(s, case, b)  # the same handle solves
        assert perf.final_residual <= TOL
    # every other preconditioner ignores the keywords
    s = make(reg, "bj", "6x6x6", preconditioner=capi.PRECOND_BJ)
    s.set_property("chebyshevDegree", 99.0)
    assert solve(s, case, b)[1].final_residual <= TOL
    # mixed precision stays refused by its own check
    s = make(reg, "mixed", "6x6x6")
    s.set_mixed_precision(True)
    with pytest.raises(capi.OglError) as e:
        solve(s, case, b)
    assert e.value.status == capi.ERR_UNSUPPORTED and "Chebyshev" in str(e.value), e.value


@pytest.mark.parametrize("fused", [1, 0])
def test_a_zero_diagonal_fails_the_solve(reg, fused):
    case, b, _ = system("6x6x6")
    broken = copy.copy(case)
    broken.diag = case.diag.copy()
    broken.diag[5] = 0.0
    assert cw.Walk(_oracle(), *oracle_csr(_oracle(), broken)).table.breakdown
    s = make(reg, "zero", "6x6x6", fused=fused, max_iter=5)
    with pytest.raises(capi.OglError) as e:
        solve(s, broken, b)
    assert e.value.status == capi.ERR_INVALID and "Chebyshev" in str(e.value), e.value
    assert s.get_property("chebyshevLambdaMaxInUse") == float("inf")
    x, perf = solve(make(reg, "zero", "6x6x6", fused=fused), case, b)  # the same handle solves afterwards
    assert perf.final_residual <= TOL and np.isfinite(x).all()
    assert s.get_property("chebyshevLambdaMaxInUse") == walk("6x6x6").table.lambda_max


# ---------------------------------------------------------------- (b) the apply

@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_apply_bits(reg, layout):
    name, kw, half = LAYOUTS[layout]
    case, b, _ = system(name)
    r = rhs(case.n_cells)
    for degree in DEGREES:
        for fused in (1, 0):
            s = make(reg, f"apply_{fused}", name, degree, fused, max_iter=2, **kw)
            solve(s, case, b)
            assert s.get_property("symmetricHalf") == float(half), layout
            if half:
                assert s.get_property("symmetricHalfPerChunk") == 0.0 and s.get_property("spmvLayout") == 2.0
            if "renumber" in kw:
                assert s.renumbering() is not None
            runs_fused = bool(half and fused)
            assert s.get_property("chebyshevFusedInUse") == float(runs_fused), (layout, degree, fused)
            assert s.get_property("chebyshevLaunchesPerApply") == (degree + 1 if runs_fused else 2 * degree + 1)
            _, apply = walk_of(s, name, degree=degree)
            np.testing.assert_array_equal(s.apply_preconditioner(r), apply(r), err_msg=f"{layout} degree {degree} fused {fused}")


def test_the_streaming_instantiations_give_the_same_bits(reg):
    """streamAboveBytes 0 puts the small systems on the STREAM kernels: FAST (12^3) and not (9x9x7)."""
    for name in ("12x12x12", "9x9x7"):
        case, b, _ = system(name)
        r = rhs(case.n_cells)
        for fused in (1, 0):
            s = make(reg, f"stream_{fused}", name, 3, fused, max_iter=2)
            s.set_property("streamAboveBytes", 0.0)
            solve(s, case, b)
            assert s.get_property("chebyshevFusedInUse") == float(fused)
            np.testing.assert_array_equal(s.apply_preconditioner(r), walk(name, degree=3).apply(r), err_msg=f"{name} {fused}")


# ---------------------------------------------------------------- (c) whole solves

def assert_is_the_oracles(s, x, perf, ref, bicgstab=False):
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)
    assert perf.n_iterations == (ref.n_iterations // 2 if bicgstab else ref.n_iterations)
    assert perf.n_norm_evals == ref.n_evals
    assert perf.initial_residual == ref.initial_residual and perf.final_residual == ref.final_residual
    assert perf.norm_factor == ref.norm_factor


@functools.lru_cache(maxsize=None)
def reference(name, solver, degree=cw.DEFAULT_DEGREE, ortho="mgs"):
    """The oracle's solve in the device's reduction tree with the walk called back; degree 0: scalar Jacobi."""
    oracle = _oracle()
    _, b, csr = system(name)
    kw = dict(tolerance=TOL, rel_tol=0.0, max_iter=300)
    with blocked(oracle, chunk_rows()):
        if solver == "gmres" and ortho != "mgs":
            return gw.gmres_walk(oracle, *csr, b, np.zeros_like(b), walk(name, degree), ortho=ortho, krylov_dim=10, **kw)
        P = walk(name, degree).precond() if degree else oracle.jacobi_generate_scalar(*csr)
        A = oracle.DistMatrix(*csr)
        if solver == "gmres":
            return oracle.gmres(A, b, np.zeros_like(b), P, krylov_dim=10, **kw)
        return getattr(oracle, solver)(A, b, np.zeros_like(b), P, **kw)


@pytest.mark.parametrize("name", list(BOXES))
@pytest.mark.parametrize("variant", ["fused", "unfused", "csr"])
def test_cg_is_the_oracles(reg, name, variant):
    case, b, _ = system(name)
    s = make(reg, f"cg_{variant}", name, fused=int(variant == "fused"), **(CSR if variant == "csr" else {}))
    x, perf = solve(s, case, b)
    assert s.get_property("chebyshevFusedInUse") == float(variant == "fused")
    ref = reference(name, "cg")
    assert ref.final_residual <= TOL and ref.n_iterations >= 5, (ref.n_iterations, ref.final_residual)
    assert_is_the_oracles(s, x, perf, ref)
    # at most four tenths of scalar Jacobi's checks on the same system
    jac = reference(name, "cg", 0)
    print(name, variant, "checks: BJ(1)", jac.n_iterations, "Chebyshev(4)", perf.n_iterations)
    assert perf.n_iterations <= 0.4 * jac.n_iterations, (perf.n_iterations, jac.n_iterations)


def test_bicgstab_on_the_random_system_is_the_oracles(reg):
    case, b, _ = system("random")
    s = make(reg, "bicg", "random")
    x, perf = solve(s, case, b)
    ref = reference("random", "bicgstab")
    assert ref.final_residual <= TOL and ref.n_iterations >= 4, (ref.n_iterations, ref.final_residual)
    assert_is_the_oracles(s, x, perf, ref, bicgstab=True)


@pytest.mark.parametrize("ortho", ["mgs", "cgs2"])
@pytest.mark.parametrize("name", ["10x9x7", "12x12x12"])
def test_gmres10_is_the_oracles(reg, name, ortho):
    case, b, _ = system(name)
    s = make(reg, f"gmres_{ortho}", name, solver=capi.SOLVER_GMRES, krylov_dim=10)
    s.set_ortho_method(ortho)
    x, perf = solve(s, case, b)
    ref = reference(name, "gmres", ortho=ortho)
    assert ref.final_residual <= TOL and 10 < ref.n_iterations < 300, (ref.n_iterations, ref.final_residual)  # (a restart)
    assert_is_the_oracles(s, x, perf, ref)


def test_a_stored_object_is_applied_with_its_stale_table(reg):
    """caching 2 over three solves with changing coefficients: solves 1 and 2 apply the object of solve 0 -- its w and its
    table -- with their own matrix in the products."""
    base = system("10x9x7")[0]
    r = rhs(base.n_cells)
    b = np.ones(base.n_cells)
    first = None
    for step in range(3):
        case = copy.copy(base)
        case.diag = base.diag * (1.0 + 0.25 * step)
        s = make(reg, "cached", "10x9x7", caching=2)
        solve(s, case, b)
        csr = oracle_csr(_oracle(), case)
        if step == 0:
            first = cw.Walk(_oracle(), *csr)
        assert s.get_property("chebyshevLambdaMaxInUse") == first.table.lambda_max
        assert first.table.lambda_max != cw.bound(*csr) or step == 0
        np.testing.assert_array_equal(s.apply_preconditioner(r), first.on_matrix(*csr).apply(r), err_msg=f"step {step}")


def test_time_steps_leave_no_memory_behind():
    """Eight time steps with new coefficients and a generation each, fused and unfused in turn on two fields: the ledger
    stands still from the second step on, and nothing is left after close."""
    base, b, _ = system("12x12x12")
    before = capi.memory_ledger().as_dict()
    reg = capi.Registry()
    marks = {}
    for step in range(8):
        case = copy.copy(base)
        case.diag = base.diag * (1.0 + 0.125 * step)
        for fused in (1, 0):
            _, perf = solve(make(reg, f"steps_{fused}", "12x12x12", fused=fused), case, b)
            assert perf.final_residual <= TOL
        if step in (1, 7):
            marks[step] = capi.memory_ledger().as_dict()
    reg.close()
    for k in soak_worker.LEDGER_EXACT:
        assert marks[7][k] == marks[1][k], (k, marks)
    after = capi.memory_ledger().as_dict()
    assert after["device_bytes"] == before["device_bytes"] and after["device_blocks"] == before["device_blocks"]


# ---------------------------------------------------------------- (d) several ranks

@pytest.mark.parametrize("mode", ["gpu-host", "gpu-peer"])
def test_two_ranks(mode):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "chebyshev_ranks_worker.py"), "--mode", mode]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    assert p.stdout.count(" ok") == 2, p.stdout
