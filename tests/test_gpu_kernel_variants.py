"""Kernel variants that a chunk count or a property selects, at the edges of their work mapping, against the oracle run in
the device's reduction tree: the leader turn of GKOCG (k_cg_step1x_fin<true>, k_cg_step2r_fin<true, 2> with two chunks per
workgroup, k_cg_turn_sym<.., LEAD>) around its 48-chunk threshold and at odd chunk counts, its second tile of partials
(lead_wave_sums, above 32,768 partials), and the BiCGStab / GMRES folds at the same edges.  Every test also asserts the
properties that prove the variant it names ran."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_matrix

pytestmark = pytest.mark.gpu

CHUNK = 512
BJ4, ISAI = "bj4", "isai"
# rows -> whether the leader turn is forced (fusedFinMaxChunks 0); the last two run with the defaults
EDGES = {
    47 * CHUNK: True,          # 47 chunks: below 3 * FIN_WAVES, no leader
    48 * CHUNK: True,          # the threshold: 24 workgroups of step_2r, 16 of them leaders
    48 * CHUNK + 1: True,      # 49 chunks, the last one of one row: the last workgroup holds one real chunk
    49 * CHUNK: True,          # odd count, full chunks
    50 * CHUNK - 1: True,        # even count, the last thread pair holds one row
    1024 * CHUNK: False,       # the last fused-finaliser size
    1024 * CHUNK + 1: False,   # the first leader size, odd
}


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


_systems = {}


def line(oracle, rows, symmetric=True):
    """A line of `rows` cells (banded: half storage applies) with its oracle matrix and preconditioners."""
    key = (rows, symmetric)
    if key not in _systems:
        case = synthetic.poisson_block(rows, 1, 1, symmetric=symmetric)
        b = synthetic.rhs_for_x_star(case)[0]
        A, (rp, cols, vals) = oracle_matrix(oracle, case)
        _systems[key] = (case, b, A, (rp, cols, vals))
    return _systems[key]


def oracle_precond(oracle, csr, pc):
    rp, cols, vals = csr
    if pc is None:
        return None
    if pc == capi.PRECOND_BJ:
        return oracle.jacobi_generate_scalar(rp, cols, vals)
    if pc == BJ4:
        return oracle.Precond(rp, cols, vals, 4)
    if pc == ISAI:
        return oracle.Precond(rp, cols, vals, isai="spd")
    return oracle.Precond(rp, cols, vals, isai="general")


def device_precond(pc):
    return {None: dict(preconditioner=capi.PRECOND_NONE), capi.PRECOND_BJ: dict(preconditioner=capi.PRECOND_BJ),
            BJ4: dict(preconditioner=capi.PRECOND_BJ, max_block_size=4),
            ISAI: dict(preconditioner=capi.PRECOND_ISAI)}[pc]


def cg_solver(reg, name, case, forced, props=(), **kw):
    cfg = capi.default_config(solver=capi.SOLVER_CG, export_res=1, adapt_min_iter=0, update_init_guess=1, **kw)
    s = reg.solver(name, cfg)
    if forced:
        s.set_property("fusedFinMaxChunks", 0.0)
        s.set_property("leadFinalizers", 1.0)
    for k, v in props:
        s.set_property(k, v)
    return s.set_matrix(case)


def expect_turn(s, rows, forced, pc=None):
    """The turn the chunk count selects: leader from 48 chunks on when forced, else from 1,025 chunks on (below that,
    the fused finalisers for the identity and scalar Jacobi, the five-launch turn for a materialised z)."""
    nc = -(-rows // CHUNK)
    lead = nc >= 48 if forced else nc > 1024
    assert s.get_property("leadFinalizersInUse") == (1.0 if lead else 0.0)
    fused = not forced and not lead and pc in (None, capi.PRECOND_BJ)
    assert s.get_property("fusedFinalizersInUse") == (1.0 if fused else 0.0)
    return lead


def cg_params():
    out = []
    for rows, forced in EDGES.items():
        for pc in (None, capi.PRECOND_BJ, BJ4, ISAI):
            for merged in ((0.0, 1.0) if pc in (None, capi.PRECOND_BJ) else (0.0,)):
                for early in ((1.0, 0.0) if forced or rows > 1024 * CHUNK else (1.0,)):
                    for max_iter in (16, 17):
                        out.append(pytest.param(rows, forced, pc, merged, early, max_iter,
                                                id=f"{rows}-{pc or 'none'}-m{int(merged)}-e{int(early)}-{max_iter}"))
    return out


@pytest.mark.parametrize("rows,forced,pc,merged,early,max_iter", cg_params())
def test_cg_leader_turn_at_launch_shape_edges(reg, oracle, rows, forced, pc, merged, early, max_iter):
    """fusedTurnBig 0 / 1 (k_cg_turn_sym<.., LEAD> on half storage), leadEarlyLoads 0 / 1 (rows loaded after the mailbox
    wait), scalar / block / ISAI preconditioner (the materialised-z leader turn), an odd and an even number of turns (the
    deferred x update of the three-launch turn)."""
    case, b, A, csr = line(oracle, rows)
    s = cg_solver(reg, f"edge_{rows}_{pc}_{merged}_{early}_{max_iter}", case, forced,
                  props=[("fusedTurn", merged), ("fusedTurnBig", merged), ("leadEarlyLoads", early)],
                  tolerance=0.0, rel_tol=0.0, max_iter=max_iter, **device_precond(pc))
    x, perf = s.solve(b, np.zeros_like(b))
    expect_turn(s, rows, forced, pc)
    assert s.get_property("fusedTurnInUse") == merged
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), oracle_precond(oracle, csr, pc), tolerance=0.0, rel_tol=0.0,
                        max_iter=max_iter)
    assert perf.n_iterations == ref.n_iterations == max_iter + 1
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)


@pytest.mark.parametrize("rows", [48 * CHUNK + 1, 49 * CHUNK, 1024 * CHUNK + 1])
@pytest.mark.parametrize("pc", [capi.PRECOND_BJ, BJ4])
@pytest.mark.parametrize("early", [1.0, 0.0])
def test_cg_leader_turn_stops_by_tolerance(reg, oracle, rows, pc, early):
    """A tolerance stop with evalFrequency 3: the turn the criterion stops at need not be one where x was brought up to
    date (deferred x update).  The tolerance is a value of the history itself, so the stop is inside the run."""
    case, b, A, csr = line(oracle, rows)
    P = oracle_precond(oracle, csr, pc)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        probe = oracle.cg(A, b, np.zeros_like(b), P, tolerance=0.0, rel_tol=0.0, max_iter=40)
        tol = float(probe.history[26])
        ref = oracle.cg(A, b, np.zeros_like(b), P, tolerance=tol, rel_tol=0.0, max_iter=600, frequency=3)
    forced = rows <= 1024 * CHUNK
    s = cg_solver(reg, f"edge_tol_{rows}_{pc}_{early}", case, forced, props=[("leadEarlyLoads", early)], tolerance=tol,
                  rel_tol=0.0, max_iter=600, eval_frequency=3, **device_precond(pc))
    x, perf = s.solve(b, np.zeros_like(b))
    assert expect_turn(s, rows, forced, pc)
    assert 3 < ref.n_iterations < 600
    assert perf.n_iterations == ref.n_iterations
    np.testing.assert_array_equal(x, ref.x)


@pytest.mark.parametrize("rows", [48 * CHUNK + 1, 49 * CHUNK])
@pytest.mark.parametrize("merged", [0.0, 1.0])
def test_cg_leader_turn_replayed_as_a_graph(reg, oracle, rows, merged):
    """hipGraph on and off at odd chunk counts: batches of leader turns captured and replayed carry the oracle's bits."""
    case, b, A, csr = line(oracle, rows)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, b, np.zeros_like(b), oracle_precond(oracle, csr, capi.PRECOND_BJ), tolerance=0.0, rel_tol=0.0,
                        max_iter=41)
    for graph in (1.0, 0.0):
        s = cg_solver(reg, f"edge_graph_{rows}_{merged}_{graph}", case, True,
                      props=[("fusedTurnBig", merged), ("hipGraph", graph)], tolerance=0.0, rel_tol=0.0, max_iter=41,
                      preconditioner=capi.PRECOND_BJ)
        x, perf = s.solve(b, np.zeros_like(b))
        assert expect_turn(s, rows, True) and s.get_property("fusedTurnInUse") == merged
        if graph:
            assert s.get_property("hipGraphCaptures") >= 1.0
        assert perf.n_iterations == ref.n_iterations == 42
        np.testing.assert_array_equal(s.history(), ref.history)
        np.testing.assert_array_equal(x, ref.x)


# ---- GKOBiCGStab and GKOGMRES at the same edges ----
@pytest.mark.parametrize("rows", [48 * CHUNK + 1, 49 * CHUNK])
@pytest.mark.parametrize("pc", [None, capi.PRECOND_BJ])
@pytest.mark.parametrize("fold,merged_check", [(1.0, 1.0), (0.0, 1.0), (0.0, 0.0)],
                         ids=["fold-lead", "turn-merged-check", "turn-own-check"])
@pytest.mark.parametrize("max_iter", [8, 9])
def test_bicgstab_turns_at_launch_shape_edges(reg, oracle, rows, pc, fold, merged_check, max_iter):
    """bicgFold 1: k_bicg_fold1/2/3<true> with the leader; bicgFold 0: the single-rank turn with the mid-turn check behind
    the second SpMV (bicgMergedCheck 1) or in a finaliser of its own (bicgMergedCheck 0)."""
    case, b, A, csr = line(oracle, rows, symmetric=False)
    cfg = capi.default_config(solver=capi.SOLVER_BICGSTAB, export_res=1, adapt_min_iter=0, update_init_guess=1,
                              tolerance=0.0, rel_tol=0.0, max_iter=max_iter, **device_precond(pc))
    s = reg.solver(f"edge_bicg_{rows}_{pc}_{fold}_{merged_check}_{max_iter}", cfg)
    for k, v in (("fusedFinMaxChunks", 0.0), ("leadFinalizers", 1.0), ("bicgFold", fold), ("bicgMergedCheck", merged_check)):
        s.set_property(k, v)
    s.set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("leadFinalizersInUse") == fold and s.get_property("fusedFinalizersInUse") == 0.0
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.bicgstab(A, b, np.zeros_like(b), oracle_precond(oracle, csr, pc), tolerance=0.0, rel_tol=0.0,
                              max_iter=max_iter)
    assert perf.n_iterations == ref.n_iterations // 2
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)


@pytest.mark.parametrize("rows", [48 * CHUNK + 1, 49 * CHUNK])
@pytest.mark.parametrize("pc", [None, capi.PRECOND_BJ])
@pytest.mark.parametrize("max_iter", [13, 25])
def test_gmres_leader_fold_at_launch_shape_edges(reg, oracle, rows, pc, max_iter):
    """gmresLead 1: k_gmres_mgs_fold<true>, krylovDim 10 not dividing maxIter (a partial last cycle)."""
    case, b, A, (rp, cols, vals) = line(oracle, rows, symmetric=False)
    cfg = capi.default_config(solver=capi.SOLVER_GMRES, krylov_dim=10, tolerance=0.0, rel_tol=0.0, max_iter=max_iter,
                              export_res=1, adapt_min_iter=0, update_init_guess=1, **device_precond(pc))
    s = reg.solver(f"edge_gmres_{rows}_{pc}_{max_iter}", cfg)
    for k, v in (("fusedFinMaxChunks", 0.0), ("leadFinalizers", 1.0), ("gmresLead", 1.0)):
        s.set_property(k, v)
    s.set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("leadFinalizersInUse") == 1.0 and s.get_property("fusedFinalizersInUse") == 0.0
    P = oracle.Precond(rp, cols, vals, 1) if pc else None
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.gmres(A, b, np.zeros_like(b), P, krylov_dim=10, tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    assert perf.n_iterations == ref.n_iterations
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)


# ---- the leader's second tile of partials: 260^3 = 17,576,000 rows ----
# 34,329 chunks: 34 partials per virtual thread; the second tile holds two of them for 537 of the 1,024 virtual threads
# and one for the others (at 257^3 it would hold one partial everywhere, and no order of addition inside it is seen)
BIG = 260
BIG_TURNS = 5


@pytest.fixture(scope="module")
def big_system(oracle):
    _systems.clear()  # (the lines are done with: room for the big system)
    case = synthetic.poisson_case(BIG)
    b = synthetic.rhs_for_x_star(case)[0]
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    refs = {}
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        for pc in (None, capi.PRECOND_BJ):
            refs[pc] = oracle.cg(A, b, np.zeros_like(b), inv if pc else None, tolerance=0.0, rel_tol=0.0,
                                 max_iter=BIG_TURNS)
    del A, rp, cols, vals
    return case, b, refs


@pytest.mark.parametrize("pc", [None, capi.PRECOND_BJ])
@pytest.mark.parametrize("lead", [1.0, 0.0])
def test_second_tile_of_leader_partials(big_system, pc, lead):
    """leadFinalizers 1: each leader stages a second tile of 32 partials per virtual thread (lead_wave_sums);
    leadFinalizers 0: the five-launch turn's finalisers walk 34,329 partials in five batches of 8,192."""
    case, b, refs = big_system
    nc = -(-case.n_cells // CHUNK)
    assert case.n_cells == 17_576_000 and nc == 34_329 and nc - 33 * 1024 == 537
    r = capi.Registry()
    try:
        s = cg_solver(r, "big", case, False, props=[("leadFinalizers", lead)], tolerance=0.0, rel_tol=0.0,
                      max_iter=BIG_TURNS, **device_precond(pc))
        x, perf = s.solve(b, np.zeros_like(b))
        assert s.get_property("leadFinalizersInUse") == lead and s.get_property("fusedFinalizersInUse") == 0.0
        ref = refs[pc]
        assert perf.n_iterations == ref.n_iterations == BIG_TURNS + 1
        np.testing.assert_array_equal(s.history(), ref.history)
        np.testing.assert_array_equal(x, ref.x)
    finally:
        r.close()
