"""GKOGMRES on a Krylov basis stored in fp32 (property basisPrecision 1 = single with orthoMethod cgs | cgs2;
kernels_gmres.hip, k_gmres_head_f32) against the NumPy walk of the contract
(tests/gmres_basis_walk.py, pinned by tests/test_gmres_basis_walk.py): exported history, x, counts, residuals and norm
factor bit for bit through the C ABI -- below one chunk, on a partial last chunk, above FUSED_FIN_MAX_CHUNKS; every
preconditioner path of the turn; restarts and partial cycles; every count of held basis vectors; the one-row tail of a
pair of floats; a renumbered device copy and the in-loop layouts; a stop by tolerance; the refusals; the basis buffers over
the life of a handle."""
import gc

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_matrix_renumbered, oracle_precond_renumbered, to_new
from mixed_walk import meets_criterion
import gmres_ortho_walk as gw
import gmres_basis_walk as bw
import soak_worker

pytestmark = pytest.mark.gpu

SHAPES = {"7x7x7": (7, 7, 7),        # 343 rows: less than one chunk; the last pair holds one row
          "13x9x11": (13, 9, 11),    # 1,287 rows: three chunks, the last partial
          "81x81x81": (81, 81, 81),  # 531,441 rows: 1,038 chunks, above FUSED_FIN_MAX_CHUNKS = 1024
          "513x1x1": (513, 1, 1)}    # a line: the second chunk is one row, the one-row tail of the float pair
BOXES = ["7x7x7", "13x9x11", "81x81x81"]
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


def walk(oracle, chunk_rows, shape, sym, precond, ortho, basis, **kw):
    """The contract's walk, computed once per set of arguments and left unchanged."""
    key = (shape, sym, precond, ortho, basis, tuple(sorted(kw.items())))
    if key not in _walks:
        (rp, cols, vals), b = system(oracle, shape, sym)[2:]
        with blocked(oracle, chunk_rows):
            _walks[key] = bw.gmres_walk(oracle, rp, cols, vals, b, np.zeros_like(b), precond_of(oracle, shape, sym, precond),
                                        ortho, basis, **kw)
    return _walks[key]


def gmres_cfg(precond="none", **kw):
    kind, block = PRECONDS[precond]
    base = dict(solver=capi.SOLVER_GMRES, preconditioner=kind, max_block_size=block, export_res=1, adapt_min_iter=0,
                update_init_guess=1, matrix_format=capi.FORMAT_CSR)
    base.update(kw)
    return capi.default_config(**base)


def device(reg, oracle, name, shape, sym, precond, ortho, basis, props=(), **kw):
    arrays, _, _, b = system(oracle, shape, sym)
    s = reg.solver(name, gmres_cfg(precond, **kw)).set_matrix(arrays)
    s.set_ortho_method(ortho)
    for key, value in props:
        s.set_property(key, value)
    if basis is not None:
        s.set_basis_precision(basis)
    x, perf = s.solve(b, np.zeros_like(b))
    return s, x, perf


def assert_same_bits(s, x, perf, w, basis="single", msg=""):
    assert s.get_property("basisPrecisionInUse") == bw.BASIS_CODE[basis], msg
    assert w.subnormal_stores == 0, msg  # (a store below 2^-126 is not pinned: the comparison needs a system without one)
    assert (perf.n_iterations, perf.n_norm_evals) == (w.n_iterations, w.n_evals), msg
    np.testing.assert_array_equal(s.history(), w.history, err_msg=msg)
    np.testing.assert_array_equal(x, w.x, err_msg=msg)
    assert (perf.initial_residual, perf.final_residual, perf.norm_factor) == (w.initial_residual, w.final_residual,
                                                                              w.norm_factor), msg


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("krylov_dim", [1, 5, 30])
@pytest.mark.parametrize("precond", list(PRECONDS))
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("shape", BOXES)
def test_device_is_the_walk(reg, oracle, chunk_rows, shape, sym, precond, krylov_dim, ortho):
    """12 turns: a restart every turn (krylovDim 1), two full cycles and a partial third (5), a partial first cycle with
    up to 12 basis vectors, i.e. two batches of eight in the kernels (30).  BJ1 is the head kernel with the inverse
    diagonal, BJ4 the materialised-z path.  On the parent of this feature the property is unknown and the solve runs on
    the double basis, whose bits differ (tests/test_gmres_basis_walk.py)."""
    kw = dict(max_iter=12, krylov_dim=krylov_dim, **BITS)
    s, x, perf = device(reg, oracle, f"gsb_{shape}_{sym}_{precond}", shape, sym, precond, ortho, "single", **kw)
    assert s.get_property("basisPrecisionInUse") == 1
    assert s.get_property("orthoMethodInUse") == gw.ORTHO_CODE[ortho]
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, shape, sym, precond, ortho, "single", **kw))


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
def test_every_count_of_basis_vectors(reg, oracle, chunk_rows, ortho, shape="13x9x11"):
    """One cycle of krylovDim 40: 1 .. 40 basis vectors.  cgs2's first update holds the floats of up to 8, 16 or 32 of them
    in registers (three instantiations) and reads them a second time beyond 32; the passes of both methods run 1 .. 5
    batches of eight."""
    kw = dict(max_iter=40, krylov_dim=40, **BITS)
    s, x, perf = device(reg, oracle, f"gsb_{shape}_False_BJ1", shape, False, "BJ1", ortho, "single", **kw)
    assert perf.n_iterations == 41
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, shape, False, "BJ1", ortho, "single", **kw))


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("precond", ["none", "BJ1"])
@pytest.mark.parametrize("shape", ["7x7x7", "513x1x1"])
def test_one_row_tail_of_the_float_pair(reg, oracle, chunk_rows, shape, precond, ortho):
    """An odd row count whose last pair holds one row (343: thread 171 of the only chunk; 513: thread 0 of the second
    chunk): the scalar path of ld2 / st2 on floats, and a leading dimension that is not the row count.  Two cycles and a
    partial one of krylovDim 9 (two batches in the last columns)."""
    kw = dict(max_iter=20, krylov_dim=9, **BITS)
    s, x, perf = device(reg, oracle, f"gsb_tail_{shape}_{precond}", shape, False, precond, ortho, "single", **kw)
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, shape, False, precond, ortho, "single", **kw))


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("precond", ["BJ1", "BJ4"])
def test_renumbered_device_copy(reg, oracle, chunk_rows, precond, ortho):
    """renumber on: the walk on the system permuted by the numbering the library reports, with the preconditioner of the
    caller's numbering expressed there (tests/test_gpu_renumber.py)."""
    case = synthetic.renumber_case(synthetic.poisson_case(14, symmetric=False), 700)
    b = synthetic.rhs_for_x_star(case)[0]
    kw = dict(max_iter=12, krylov_dim=5, **BITS)
    s = reg.solver(f"gsb_rn_{precond}", gmres_cfg(precond, renumber=capi.RENUMBER_ON, **kw)).set_matrix(case)
    s.set_ortho_method(ortho).set_basis_precision("single")
    new_id = s.renumbering()
    assert new_id is not None
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("basisPrecisionInUse") == 1
    _, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    P = oracle_precond_renumbered(oracle, case, rp, cols, vals, new_id, PRECONDS[precond][1])
    with blocked(oracle, chunk_rows):
        w = bw.gmres_walk(oracle, rp, cols, vals, to_new(b, new_id), np.zeros_like(b), P, ortho, "single", **kw)
    assert w.subnormal_stores == 0
    assert perf.n_iterations == w.n_iterations == 13 and perf.n_norm_evals == w.n_evals
    np.testing.assert_array_equal(s.history(), w.history)
    np.testing.assert_array_equal(x, w.x[new_id])
    assert (perf.initial_residual, perf.final_residual, perf.norm_factor) == (w.initial_residual, w.final_residual,
                                                                              w.norm_factor)


# which SpMV layout runs in the loop: name -> (config, (spmvLayout, symmetricHalf)) on the symmetric 13x9x11 box
LAYOUTS = {"half": (dict(), (2.0, 1.0)), "sell": (dict(symmetric_half=0), (2.0, 0.0)),
           "csr": (dict(compress_indices=0), (0.0, 0.0))}


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_in_loop_layouts(reg, oracle, chunk_rows, layout, ortho):
    """Half storage, Sell and the CSR stream kernel write the working vector (fp64, in its own buffer) from the widened
    V_it the head kernel left: the same bits on each."""
    cfg_kw, (lay, half) = LAYOUTS[layout]
    kw = dict(max_iter=12, krylov_dim=5, **BITS)
    s, x, perf = device(reg, oracle, f"gsb_lay_{layout}", "13x9x11", True, "BJ1", ortho, "single", **cfg_kw, **kw)
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, "13x9x11", True, "BJ1", ortho, "single", **kw))


@pytest.mark.parametrize("ortho", ["cgs", "cgs2"])
def test_stop_by_tolerance(reg, oracle, chunk_rows, ortho):
    """tolerance 1e-6 on 13x9x11 asymmetric with BJ1.  maxIter is twice the turn count of the DOUBLE walk, fixed before the
    single solve runs (tests/test_gmres_basis_walk.py confirms the single walk stays inside it): the rounded basis may cost
    turns, not the answer -- the criterion holds on the true residual."""
    tol = dict(tolerance=1e-6, rel_tol=0.0, krylov_dim=30)
    d = walk(oracle, chunk_rows, "13x9x11", False, "BJ1", ortho, "double", max_iter=1000, **tol)
    assert d.n_iterations < 1000
    cap = 2 * (d.n_iterations - 1)
    s, x, perf = device(reg, oracle, "gsb_tol", "13x9x11", False, "BJ1", ortho, "single", max_iter=cap, **tol)
    (rp, cols, vals), b = system(oracle, "13x9x11", False)[2:]
    true = gw.true_residual(oracle, rp, cols, vals, b, x, perf.norm_factor)
    print(f"{ortho} on the device: double walk {d.n_iterations - 1} turns, single {perf.n_iterations - 1} (cap {cap}), "
          f"recorded {perf.final_residual:.3e}, true {true:.3e}")
    assert perf.n_iterations - 1 < cap
    assert meets_criterion(perf.final_residual, perf.initial_residual, tolerance=1e-6, rel_tol=0.0)
    assert meets_criterion(true, perf.initial_residual, tolerance=1e-6, rel_tol=0.0)
    assert_same_bits(s, x, perf, walk(oracle, chunk_rows, "13x9x11", False, "BJ1", ortho, "single", max_iter=cap, **tol))


def test_refusals(reg, oracle):
    arrays, _, _, b = system(oracle, "13x9x11", False)
    s = reg.solver("gsb_bad", gmres_cfg("BJ1", max_iter=5, krylov_dim=5, **BITS)).set_matrix(arrays)
    s.set_ortho_method("cgs")
    for bad in (2.0, -1.0, 0.5):
        s.set_property("basisPrecision", bad)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, np.zeros_like(b))
        assert e.value.status == capi.ERR_INVALID and "basisPrecision" in str(e.value)
    s.set_basis_precision("single").set_ortho_method("mgs")
    with pytest.raises(capi.OglError) as e:
        s.solve(b, np.zeros_like(b))
    assert e.value.status == capi.ERR_UNSUPPORTED
    assert "basisPrecision" in str(e.value) and "orthoMethod" in str(e.value)
    s.set_ortho_method("cgs2")
    s.solve(b, np.zeros_like(b))  # the handle goes on after a refusal
    assert s.get_property("basisPrecisionInUse") == 1.0 and s.get_property("orthoMethodInUse") == 2.0


def test_gkocg_ignores_the_keyword(reg, oracle):
    """Any value, a valid one or not: the same bits as with the property left unset."""
    arrays, _, _, b = system(oracle, "13x9x11", True)
    out = []
    for i, value in enumerate((None, 1.0, 2.0)):
        s = reg.solver(f"gsb_cg_{i}", gmres_cfg("BJ1", solver=capi.SOLVER_CG, max_iter=12, **BITS)).set_matrix(arrays)
        if value is not None:
            s.set_property("basisPrecision", value)
        x, perf = s.solve(b, np.zeros_like(b))
        out.append((x, s.history().copy(), perf.n_iterations))
    for x, hist, n in out[1:]:
        np.testing.assert_array_equal(hist, out[0][1])
        np.testing.assert_array_equal(x, out[0][0])
        assert n == out[0][2]


def basis_bytes(n, m, basis):
    """(m + 1) vectors: doubles at a leading dimension of n + 2, floats at n rounded up to a multiple of four (16 bytes)."""
    return (m + 1) * ((n + 3) // 4 * 4) * 4 if basis == "single" else (m + 1) * (n + 2) * 8


@pytest.mark.parametrize("graph", [1.0, 0.0], ids=["hipGraph", "noGraph"])
def test_double_single_double_on_one_handle(oracle, chunk_rows, graph):
    """Each solve is its own walk bit for bit, whatever the handle ran before; basisBytes halves; under the ledger the
    float basis comes with the first single solve and nothing comes or goes after it."""
    arrays, _, _, b = system(oracle, "13x9x11", False)
    n, m = b.size, 5
    kw = dict(max_iter=12, krylov_dim=m, **BITS)
    gc.collect()
    r = capi.Registry()
    try:
        marks, nbytes = [], []
        for basis in ("double", "single", "double", "single"):
            s, x, perf = device(r, oracle, "gsb_life", "13x9x11", False, "BJ1", "cgs2", basis, props=(("hipGraph", graph),), **kw)
            assert_same_bits(s, x, perf, walk(oracle, chunk_rows, "13x9x11", False, "BJ1", "cgs2", basis, **kw), basis, basis)
            nbytes.append(s.get_property("basisBytes"))
            marks.append(capi.memory_ledger().as_dict())
        assert nbytes == [basis_bytes(n, m, "double"), basis_bytes(n, m, "single")] * 2
        assert 2 * nbytes[1] <= nbytes[0] + 8 * (m + 1)  # (half, up to the padding of a float vector to 16 bytes)
        # (the first single solve adds its float basis and nothing of the size of a double one)
        assert basis_bytes(n, m, "single") <= marks[1]["device_bytes"] - marks[0]["device_bytes"] < basis_bytes(n, m, "double")
        for later in marks[2:]:
            for k in soak_worker.LEDGER_EXACT + ("device_alloc_calls", "pinned_alloc_calls"):
                assert later[k] == marks[1][k], (k, marks)
    finally:
        r.close()


def test_time_steps_alternating_precisions_leave_the_ledger_alone(oracle):
    """Ten solves on one field, double and single in turn, the handle fetched anew every step as a time-step loop does: each
    basis comes with the first step that needs it and stays; after the second step the ledger does not move."""
    arrays, _, _, b = system(oracle, "13x9x11", False)
    gc.collect()
    r = capi.Registry()
    marks = []
    for step in range(10):
        s = r.solver("gsb_steps", gmres_cfg("BJ1", max_iter=12, krylov_dim=5, **BITS)).set_matrix(arrays)
        s.set_ortho_method("cgs2").set_basis_precision("single" if step % 2 else "double")
        s.solve(b, np.zeros_like(b))
        assert s.get_property("basisPrecisionInUse") == (1.0 if step % 2 else 0.0)
        marks.append(capi.memory_ledger().as_dict())
    r.close()
    assert marks[1]["device_bytes"] > marks[0]["device_bytes"]
    for later in marks[2:]:
        for k in soak_worker.LEDGER_EXACT + ("device_alloc_calls", "pinned_alloc_calls"):
            assert later[k] == marks[1][k], (k, marks)
    assert marks[-1]["unknown_frees"] == 0


def test_a_solver_that_only_runs_single_books_no_double_basis(oracle):
    """Two fresh registries with one solve each: what the single one holds on the device is lower by at least
    (m + 1) N 4 bytes -- its basis is (m + 1) float vectors, and the working vector is a buffer both twins have."""
    arrays, _, _, b = system(oracle, "13x9x11", False)
    n, m = b.size, 30
    held = {}
    for basis in ("double", "single"):
        gc.collect()
        before = capi.memory_ledger().as_dict()["device_bytes"]
        r = capi.Registry()
        try:
            s, _, _ = device(r, oracle, "gsb_fresh", "13x9x11", False, "BJ1", "cgs", basis, max_iter=12, krylov_dim=m, **BITS)
            assert s.get_property("basisBytes") == basis_bytes(n, m, basis)
            held[basis] = s.get_property("deviceBytesInUse") - before
        finally:
            r.close()
    print(f"device bytes of a fresh solver: double {held['double']:.0f}, single {held['single']:.0f}")
    assert held["double"] - held["single"] >= (m + 1) * n * 4
