"""GKOGMRES with classical Gram-Schmidt in block form (property orthoMethod 1 = cgs, 2 = cgs2; kernels_gmres.hip,
DESIGN.md section 7d) against the NumPy walk of the contract (tests/gmres_ortho_walk.py, pinned to the oracle by
tests/test_gmres_ortho_walk.py): exported history and x bit for bit through the C ABI -- below one chunk, on a partial
last chunk, above FUSED_FIN_MAX_CHUNKS; every preconditioner path of the turn; restarts and partial cycles; stops at every
turn; a renumbered device copy; the refusals; the allocation ledger of a time-step loop that alternates the methods."""
import gc

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_matrix_renumbered, oracle_precond_renumbered, to_new
from mixed_walk import meets_criterion
import gmres_ortho_walk as gw
import soak_worker

pytestmark = pytest.mark.gpu

SHAPES = {"7x7x7": (7, 7, 7),        # 343 rows: less than one chunk
          "13x9x11": (13, 9, 11),    # 1,287 rows: three chunks, the last partial
          "81x81x81": (81, 81, 81)}  # 531,441 rows: 1,038 chunks, above FUSED_FIN_MAX_CHUNKS = 1024
PRECONDS = {"none": (capi.PRECOND_NONE, 1), "BJ1": (capi.PRECOND_BJ, 1), "BJ4": (capi.PRECOND_BJ, 4)}
BITS = dict(tolerance=0.0, rel_tol=0.0)  # a fixed number of turns


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module")
def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


_systems, _preconds, _walks = {}, {}, {}


def system(oracle, shape, sym):
    """(case as LduArrays, case, (rp, cols, vals), b) of a box, built once."""
    if (shape, sym) not in _systems:
        kw = {} if sym else dict(symmetric=False, off_upper=-0.9, off_lower=-1.1)
        case = synthetic.poisson_block(*SHAPES[shape], **kw)
        b = synthetic.rhs_for_x_star(case)[0]
        _systems[shape, sym] = (capi.LduArrays(case), case, oracle_csr(oracle, case), b)
    return _systems[shape, sym]


def precond_of(oracle, shape, sym, precond):
    kind, block = PRECONDS[precond]
    if kind == capi.PRECOND_NONE:
        return None
    if (shape, sym, precond) not in _preconds:
        rp, cols, vals = system(oracle, shape, sym)[2]
        _preconds[shape, sym, precond] = oracle.Precond(rp, cols, vals, block)
    return _preconds[shape, sym, precond]


def walk(oracle, chunk_rows, shape, sym, precond, ortho, **kw):
    """The contract's walk, computed once per set of arguments and left unchanged."""
    key = (shape, sym, precond, ortho, tuple(sorted(kw.items())))
    if key not in _walks:
        (rp, cols, vals), b = system(oracle, shape, sym)[2:]
        with blocked(oracle, chunk_rows):
            _walks[key] = gw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), precond_of(oracle, shape, sym, precond),
                                        ortho, **kw)
    return _walks[key]


def gmres_cfg(precond="none", **kw):
    kind, block = PRECONDS[precond]
    base = dict(solver=capi.SOLVER_GMRES, preconditioner=kind, max_block_size=block, export_res=1, adapt_min_iter=0,
                update_init_guess=1, matrix_format=capi.FORMAT_CSR)
    base.update(kw)
    return capi.default_config(**base)


def device(reg, oracle, name, shape, sym, precond, ortho, **kw):
    arrays, _, _, b = system(oracle, shape, sym)
    s = reg.solver(name, gmres_cfg(precond, **kw)).set_matrix(arrays)
    if ortho is not None:
        s.set_ortho_method(ortho)
    x, perf = s.solve(b, np.zeros_like(b))
    return s, x, perf


def assert_same_bits(s, x, perf, w, msg=""):
    assert (perf.n_iterations, perf.n_norm_evals) == (w.n_iterations, w.n_evals), msg
    np.testing.assert_array_equal(s.history(), w.history, err_msg=msg)
    np.testing.assert_array_equal(x, w.x, err_msg=msg)
    assert (perf.initial_residual, perf.final_residual, perf.norm_factor) == (w.initial_residual, w.final_residual,
                                                                              w.norm_factor), msg


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("krylov_dim", [1, 5, 30])
@pytest.mark.parametrize("precond", list(PRECONDS))
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_is_the_walk(reg, oracle, chunk_rows, shape, sym, precond, krylov_dim, ortho):
    """12 turns: a restart every turn (krylovDim 1), two full cycles and a partial third (5), a partial first cycle with
    up to 12 basis vectors, i.e. two batches of eight in the kernels (30).  BJ1 is the late-scaling path, BJ4 the generic
    one.  On the parent of this feature the property is unknown and the solve stays on modified Gram-Schmidt, whose bits
    differ (tests/test_gmres_ortho_walk.py::test_block_forms_are_not_mgs)."""
    kw = dict(max_iter=12, krylov_dim=krylov_dim, **BITS)
    s, x, perf = device(reg, oracle, f"gso_{shape}_{sym}_{precond}", shape, sym, precond, ortho, **kw)
    assert s.get_property("orthoMethodInUse") == gw.ORTHO_CODE[ortho]
    assert s.get_property("fusedFinalizersInUse") == 0.0
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, shape, sym, precond, ortho, **kw))


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
def test_every_count_of_basis_vectors(reg, oracle, chunk_rows, ortho, shape="13x9x11"):
    """One cycle of krylovDim 40: 1 .. 40 basis vectors.  cgs2's first update keeps the rows of up to 8, 16 or 32 of them in
    registers (three instantiations) and reads them a second time beyond 32; the passes of both methods run 1 .. 5 batches
    of eight."""
    kw = dict(max_iter=40, krylov_dim=40, **BITS)
    s, x, perf = device(reg, oracle, f"gso_{shape}_False_BJ1", shape, False, "BJ1", ortho, **kw)
    assert s.get_property("orthoMethodInUse") == gw.ORTHO_CODE[ortho] and perf.n_iterations == 41
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, shape, False, "BJ1", ortho, **kw))


def test_mgs_by_name_is_the_default_and_the_launch_counts(reg, oracle, chunk_rows):
    kw = dict(max_iter=12, krylov_dim=5, **BITS)
    s0, x0, perf0 = device(reg, oracle, "gso_default", "13x9x11", False, "BJ1", None, **kw)
    assert s0.get_property("orthoMethodInUse") == 0.0
    h0 = s0.history()
    s1, x1, perf1 = device(reg, oracle, "gso_named", "13x9x11", False, "BJ1", "mgs", **kw)
    assert s1.get_property("orthoMethodInUse") == 0.0
    np.testing.assert_array_equal(s1.history(), h0)
    np.testing.assert_array_equal(x1, x0)
    assert perf1.n_iterations == perf0.n_iterations == 13
    assert_same_bits(s1, x1, perf1, walk(oracle, chunk_rows, "13x9x11", False, "BJ1", "mgs", **kw))
    # turn_gmres: the SpMV's launch and the scaling's (k_gmres_scale_mul here) + multidot | fin_h | block_update |
    # FIN_GMRES_COL, and for cgs2 a second block_update | fin_h pair
    for ortho, launches in (("cgs", 1 + 1 + 4), ("cgs2", 1 + 1 + 6)):
        s, _, _ = device(reg, oracle, "gso_named", "13x9x11", False, "BJ1", ortho, **kw)
        assert s.get_property("orthoMethodInUse") == gw.ORTHO_CODE[ortho]
        assert s.get_property("gmresLaunchesPerTurn") == launches
    # mgs on this small system: folded links, it + 2 of them at column it and the column's finaliser: 5 launches on average
    # over a cycle of 5, + 2
    s, _, _ = device(reg, oracle, "gso_named", "13x9x11", False, "BJ1", "mgs", **kw)
    assert s.get_property("gmresLaunchesPerTurn") == 1 + 1 + 5.0


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("precond", list(PRECONDS))
def test_stops_anywhere_around_the_restarts(reg, oracle, chunk_rows, precond, ortho):
    """A stop at every turn index 1 .. 2 krylovDim + 1 for krylovDim 4: at, one before and one after every cycle boundary."""
    for max_iter in range(1, 2 * 4 + 2):
        kw = dict(max_iter=max_iter, krylov_dim=4, **BITS)
        s, x, perf = device(reg, oracle, f"gso_stop_{precond}", "13x9x11", False, precond, ortho, **kw)
        assert perf.n_iterations == max_iter + 1
        assert_same_bits(s, x, perf, walk(oracle, chunk_rows, "13x9x11", False, precond, ortho, **kw), f"maxIter {max_iter}")


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("precond", ["BJ1", "BJ4"])
def test_renumbered_device_copy(reg, oracle, chunk_rows, precond, ortho):
    """renumber on: the walk on the system permuted by the numbering the library reports, with the preconditioner of the
    caller's numbering expressed there (tests/test_gpu_renumber.py)."""
    case = synthetic.renumber_case(synthetic.poisson_case(14, symmetric=False), 700)
    b = synthetic.rhs_for_x_star(case)[0]
    kw = dict(max_iter=12, krylov_dim=5, **BITS)
    s = reg.solver(f"gso_rn_{precond}", gmres_cfg(precond, renumber=capi.RENUMBER_ON, **kw)).set_matrix(case)
    s.set_ortho_method(ortho)
    new_id = s.renumbering()
    assert new_id is not None
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("orthoMethodInUse") == gw.ORTHO_CODE[ortho]
    _, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    P = oracle_precond_renumbered(oracle, case, rp, cols, vals, new_id, PRECONDS[precond][1])
    with blocked(oracle, chunk_rows):
        w = gw.gmres_walk(oracle, rp, cols, vals, to_new(b, new_id), np.zeros_like(b), P, ortho, **kw)
    assert perf.n_iterations == w.n_iterations == 13
    np.testing.assert_array_equal(s.history(), w.history)
    np.testing.assert_array_equal(x, w.x[new_id])
    assert perf.norm_factor == w.norm_factor


def test_refusals(reg, oracle, chunk_rows):
    arrays, _, _, b = system(oracle, "13x9x11", False)
    s = reg.solver("gso_bad", gmres_cfg("BJ1", max_iter=5, krylov_dim=5, **BITS)).set_matrix(arrays)
    for bad in (3.0, -1.0, 0.5):
        s.set_property("orthoMethod", bad)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, np.zeros_like(b))
        assert e.value.status == capi.ERR_INVALID and "orthoMethod" in str(e.value)
    s.set_ortho_method("cgs")
    s.solve(b, np.zeros_like(b))  # the handle goes on after a refusal
    assert s.get_property("orthoMethodInUse") == 1.0


def test_two_ranks_are_refused(oracle):
    """A host communicator of size 2 in one process: the solve fails before anything of it is enqueued (the callbacks are
    never reached by it), and the message names the method and the rank count."""
    arrays, _, _, b = system(oracle, "7x7x7", False)
    r2 = capi.Registry()
    try:
        r2.set_host_comm(0, 2, lambda v: v, lambda nbr, cnt, send: send)
        s = r2.solver("gso_two", gmres_cfg("BJ1", max_iter=3, krylov_dim=5, **BITS)).set_matrix(arrays)
        for word in ("cgs", "cgs2"):
            s.set_ortho_method(word)
            with pytest.raises(capi.OglError) as e:
                s.solve(b, np.zeros_like(b))
            assert e.value.status == capi.ERR_UNSUPPORTED
            assert f"orthoMethod {word} " in str(e.value) and "2 ranks" in str(e.value)
    finally:
        r2.close()


@pytest.mark.parametrize("solver", [capi.SOLVER_CG, capi.SOLVER_BICGSTAB], ids=["GKOCG", "GKOBiCGStab"])
def test_other_solvers_ignore_the_keyword(reg, oracle, solver):
    """Any value, a valid one or not: the same bits as with the property left unset."""
    arrays, _, _, b = system(oracle, "13x9x11", solver == capi.SOLVER_CG)
    out = []
    for i, value in enumerate((None, 2.0, 3.0)):
        s = reg.solver(f"gso_other_{solver}_{i}", gmres_cfg("BJ1", solver=solver, max_iter=12, **BITS)).set_matrix(arrays)
        if value is not None:
            s.set_property("orthoMethod", value)
        x, perf = s.solve(b, np.zeros_like(b))
        out.append((x, s.history().copy(), perf.n_iterations))
    for x, hist, n in out[1:]:
        np.testing.assert_array_equal(hist, out[0][1])
        np.testing.assert_array_equal(x, out[0][0])
        assert n == out[0][2]


def test_time_steps_alternating_methods_leave_the_ledger_alone(oracle):
    """Five solves on one handle, mgs and cgs2 in turn: the partial array and the coefficient vector of the block form come
    with the first cgs2 step and stay; after the second step the ledger does not move."""
    arrays, _, _, b = system(oracle, "13x9x11", False)
    gc.collect()
    reg = capi.Registry()
    marks = []
    for step in range(5):
        s = reg.solver("gso_steps", gmres_cfg("BJ1", max_iter=12, krylov_dim=5, **BITS)).set_matrix(arrays)
        s.set_ortho_method("cgs2" if step % 2 else "mgs")
        s.solve(b, np.zeros_like(b))
        assert s.get_property("orthoMethodInUse") == (2.0 if step % 2 else 0.0)
        marks.append(capi.memory_ledger().as_dict())
    reg.close()
    assert marks[1]["device_bytes"] > marks[0]["device_bytes"]
    for later in marks[2:]:
        for k in soak_worker.LEDGER_EXACT + ("device_alloc_calls", "pinned_alloc_calls"):
            assert later[k] == marks[1][k], (k, marks)
    assert marks[-1]["unknown_frees"] == 0


def test_cgs2_meets_the_default_criterion_on_the_true_residual(reg, oracle, chunk_rows):
    kw = dict(tolerance=1e-6, rel_tol=1e-6)
    s, x, perf = device(reg, oracle, "gso_true", "13x9x11", False, "BJ1", "cgs2", max_iter=1000, krylov_dim=30, **kw)
    (rp, cols, vals), b = system(oracle, "13x9x11", False)[2:]
    assert perf.n_iterations < 1000 and meets_criterion(perf.final_residual, perf.initial_residual, **kw)
    true = gw.true_residual(oracle, rp, cols, vals, b, x, perf.norm_factor)
    print(f"cgs2 on the device: {perf.n_iterations} checks, recorded {perf.final_residual:.3e}, true {true:.3e}")
    assert meets_criterion(true, perf.initial_residual, **kw)
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, "13x9x11", False, "BJ1", "cgs2", max_iter=1000, krylov_dim=30, **kw))
