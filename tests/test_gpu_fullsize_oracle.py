"""The headline configuration itself under the oracle: everything below runs at the sizes
BASELINE.json quotes -- not toy sizes with the big-system kernels forced on -- with every library default left
alone, and is compared BIT FOR BIT with the oracle run in the device's reduction tree (orc_set_reduction(BLOCKED)),
plus a stated bound against the oracle in the reference executor's left-to-right order.

  (a) reductions at n = 10,077,696: dot / norm1 / sum (19,683 per-chunk partials -> the finaliser's second and third
      batches of 8,192, device_common.hpp reduce_partials)
  (b) GKOCG + BJ and GKOCG (none) at 216^3, 30 turns: matrix, history, x, norm factor, iteration count
      (the STREAM instantiation of the half-storage SpMV with the band-aware workgroup order, inside a solve)
      on the held-z turn, which these sizes run by default (asserted: heldZInUse, heldZGridInUse), and one 216^3 solve
      stopped by its tolerance at evalFrequency 3, against the three-launch turn
  (c) 136^3 (one rank's share of configs[3]) with the merged step_1x + SpMV kernel ON BY DEFAULT, and 100^3
      (rows not a multiple of the chunk: the clamped tail gathers); 128^3 non-symmetric GKOBiCGStab + BJ
  (d) the first restart cycle of GKOGMRES(30) + BJ at 184^3 with shuffled cells (one rank's share of configs[4]),
      against the oracle on the numbering the library reports
  (e) the reference's gtest vectors (unitTests/test_HostMatrix.C:8-107 -> tests/golden/host_matrix_kat.json) through
      ogl_solver_set_matrix -> ogl_solver_get_local_matrix, i.e. through the DEVICE set-up kernels, compared with the
      JSON directly

  (f) BASELINE configs[2]'s keyword pair at its size: GKOBiCGStab + ISAI and + GISAI on ~2 M unstructured cells (128^3
      cells shuffled in windows of 65536 -- `renumber auto` renumbers, ISAI(spd)'s W keeps the CALLER's triangle and runs
      on the compressed layout with its rows sorted by length inside the wavefront windows -- and a three-block
      blockMesh of 2.06 M cells), first 10 turns: history, x, iteration count bit-equal on the reported numbering

The oracle needs 0.3-0.4 s per CG turn at 10 M rows on one host core; the whole file runs in about three minutes.
Reference: StoppingCriterion/StoppingCriterion.C:71-151 (what a history entry is), lduLduBase/lduLduBase.H:189-308.
"""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import (blocked, oracle_csr, oracle_matrix, oracle_matrix_renumbered, oracle_precond_renumbered, rel_dev,
                     to_new)

pytestmark = pytest.mark.gpu

TURNS = 30
# Against the SEQUENTIAL oracle (the reference executor's order) over the first 30 turns at 10 M rows.  north_star
# asks for 1e-12; two summation orders of the same 10 M products already differ by a few 1e-13 per dot and CG
# carries that forward: measured 2.2e-12 (BJ) over these 31 checks (2.6e-12 over 50 turns).
SEQ_BOUND_216 = 5e-12


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


@pytest.fixture(scope="module")
def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


def resident_grid():
    """Four workgroups per compute unit: the grid of the held-z turn when nothing lowers it (1,024 on MI355X)."""
    import torch
    return 4.0 * torch.cuda.get_device_properties(0).multi_processor_count


def cfg(**kw):
    base = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_BJ, tolerance=0.0, rel_tol=0.0,
                max_iter=TURNS, export_res=1, adapt_min_iter=0, matrix_format=capi.FORMAT_CSR)
    base.update(kw)
    return capi.default_config(**base)


@pytest.fixture(scope="module")
def big(oracle):
    """216^3: the case, the oracle's matrix of it (its own LDU conversion) and b = A x*."""
    case = synthetic.poisson_case(216)
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    xs = synthetic.x_star(case.global_index, case.global_n)
    b = oracle.spmv(rp, cols, vals, xs)
    return case, A, (rp, cols, vals), b


# ------------------------------------------------------------------------------------------ (a)

def test_reductions_at_10m_rows_bit_equal(reg, oracle, chunk_rows, big):
    case = big[0]
    n = case.n_cells
    assert n == 10077696 and (n + chunk_rows - 1) // chunk_rows > 2 * 8192     # three batches of partials
    s = reg.solver("p", cfg()).set_matrix(case)
    rng = np.random.default_rng(20241016)
    a, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    with blocked(oracle, chunk_rows):
        assert s.reduce("dot", a, b) == oracle.dot(a, b)
        assert s.reduce("norm1", a) == oracle.norm1(a)
        assert s.reduce("sum", a) == oracle.vsum(a)
    # the left-to-right sums of the reference executor: rounding-level agreement
    assert s.reduce("dot", a, b) == pytest.approx(oracle.dot(a, b), rel=1e-11, abs=1e-9)
    assert s.reduce("norm1", a) == pytest.approx(oracle.norm1(a), rel=1e-12)


# ------------------------------------------------------------------------------------------ (b)

def test_device_matrix_at_216_is_the_oracles(reg, big):
    case, A, (rp, cols, vals), b = big
    s = reg.solver("p", cfg()).set_matrix(case)
    d_rp, d_cols, d_map, d_vals = s.local_matrix()
    np.testing.assert_array_equal(d_rp, rp)
    np.testing.assert_array_equal(d_cols, cols)
    np.testing.assert_array_equal(d_vals, vals)


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE], ids=["BJ", "none"])
def test_cg_216_history_bit_equal(reg, oracle, chunk_rows, big, precond):
    case, A, (rp, cols, vals), b = big
    s = reg.solver("p" if precond else "p_none", cfg(preconditioner=precond)).set_matrix(case)
    s.upload_solution(None)
    x, perf = s.solve(b, np.zeros_like(b))
    hist = s.history()
    # every default left alone: the half storage, its STREAM instantiation (matrix + vectors exceed the Infinity
    # Cache) and the held-z turn of two launches (SpMV | k_cg_step2r1x) on the device's full resident grid, every
    # workgroup of it with 19 or 20 chunks -- what bench.py times
    assert s.get_property("symmetricHalf") == 1.0 and s.get_property("symmetricHalfPerChunk") == 0.0
    assert s.get_property("fusedTurnInUse") == 0.0 and s.get_property("fusedFinalizersInUse") == 0.0
    assert s.get_property("leadFinalizersInUse") == 1.0
    assert s.get_property("heldZInUse") == 1.0 and s.get_property("heldZGridInUse") == resident_grid()
    inv = oracle.jacobi_generate_scalar(rp, cols, vals) if precond else None
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=TURNS)
    with blocked(oracle, chunk_rows):
        ref = oracle.cg(A, b, np.zeros_like(b), inv, **kw)
    assert perf.n_iterations == ref.n_iterations == TURNS + 1
    np.testing.assert_array_equal(hist, ref.history)
    np.testing.assert_array_equal(x, ref.x)
    assert perf.norm_factor == ref.norm_factor
    assert perf.initial_residual == ref.initial_residual and perf.final_residual == ref.final_residual
    seq = oracle.cg(A, b, np.zeros_like(b), inv, **kw)
    assert seq.n_iterations == ref.n_iterations
    dev = rel_dev(hist, seq.history)
    print(f"216^3 {'BJ' if precond else 'none'}: max rel deviation from the sequential order over "
          f"{hist.size} checks {dev.max():.2e} (first 5: {dev[:5].max():.2e})")
    assert dev.max() <= SEQ_BOUND_216
    assert dev[:5].max() <= 1e-12
    assert rel_dev(perf.norm_factor, seq.norm_factor) <= 1e-12


def test_cg_216_stops_by_tolerance_on_the_held_z_turn(reg, big):
    """The only tests at full load stop by max_iter: here the criterion inside k_cg_step2r1x ends a 216^3 solve by its
    tolerance, at evalFrequency 3, with 19 or 20 chunks in every workgroup -- against the three-launch turn (heldZ 0); the
    oracle would need minutes for this many turns at 10 M rows.  The tolerance is a value of the history itself: this
    history rises above its first value and stays there for more than 45 turns, so a residual of turn 20 would stop the
    solve at turn 0; it is the first record low from turn 20 on (of a probe run without tolerance), which puts the stop
    inside the run by construction."""
    case, A, (rp, cols, vals), b = big
    probe = reg.solver("p_tol_off", cfg(max_iter=300)).set_matrix(case)
    probe.set_property("heldZ", 0.0)
    probe.upload_solution(None)
    probe.solve(b, np.zeros_like(b))
    h = probe.history()
    k = next(k for k in range(20, h.size) if h[k] < h[:k].min())
    out = {}
    for held, name in ((1.0, "p_tol_on"), (0.0, "p_tol_off")):
        s = reg.solver(name, cfg(tolerance=float(h[k]), max_iter=600, eval_frequency=3)).set_matrix(case)
        s.set_property("heldZ", held)
        s.upload_solution(None)
        x, perf = s.solve(b, np.zeros_like(b))
        assert s.get_property("heldZInUse") == held and s.get_property("leadFinalizersInUse") == 1.0
        assert s.get_property("heldZGridInUse") == (resident_grid() if held else 0.0)
        out[held] = (x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals)
    on, off = out[1.0], out[0.0]
    print(f"216^3: tolerance {h[k]:.6e} = the residual of turn {k}, stop after {on[1]} checks")
    assert k < on[1] < 600 and on[1] % 3 == 1 and on[3] < h[k]
    assert on[1] == off[1] and on[3] == off[3] and on[4] == off[4]
    np.testing.assert_array_equal(on[2], off[2])
    np.testing.assert_array_equal(on[0], off[0])


# ------------------------------------------------------------------------------------------ (c)

@pytest.mark.parametrize("edge,merged", [(136, True), (100, True), (160, False)])
def test_cg_default_turn_kernels_bit_equal(reg, oracle, chunk_rows, edge, merged):
    """136^3 = one rank's share of configs[3]: the merged step_1x + SpMV kernel (k_cg_turn_sym_big) is what runs by
    default while matrix + vectors fit the Infinity Cache.  100^3: 1,000,000 rows = 1953 chunks + 64 rows (the tail
    lanes of the last chunk gather at clamped indices).  160^3: the merged kernel stands down (streamed) and the held-z
    turn takes over by default, on the full resident grid (8,000 chunks: 7 or 8 per workgroup, registers only); at the
    cache-resident sizes it stays off."""
    case = synthetic.poisson_case(edge)
    s = reg.solver(f"c{edge}", cfg()).set_matrix(case)
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    b = oracle.spmv(rp, cols, vals, synthetic.x_star(case.global_index, case.global_n))
    x, perf = s.solve(b, np.zeros_like(b))
    assert s.get_property("fusedTurnInUse") == (1.0 if merged else 0.0)
    assert s.get_property("fusedFinalizersInUse") == 0.0
    assert s.get_property("heldZInUse") == (0.0 if merged else 1.0)
    assert s.get_property("heldZGridInUse") == (0.0 if merged else resident_grid())
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    with blocked(oracle, chunk_rows):
        ref = oracle.cg(A, b, np.zeros_like(b), inv, tolerance=0.0, rel_tol=0.0, max_iter=TURNS)
    assert perf.n_iterations == ref.n_iterations
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)
    assert perf.norm_factor == ref.norm_factor


@pytest.mark.parametrize("gx,gy,gz", [(27, 19, 1), (5, 103, 1), (3, 11, 31), (7, 73, 1),        # n % 512 = 1, 3, 511, 511
                                      (2, 257, 1), (14, 73, 1), (6, 5, 17), (64, 32, 17)],    # even lines: 2, 510, 510, 0
                         ids=lambda v: str(v))
def test_half_storage_tail_chunks(reg, oracle, chunk_rows, gx, gy, gz):
    """Row counts with n % 512 in {0, 1, 2, 3, 510, 511}: the last chunk's idle lanes issue their (discarded)
    gathers at indices clamped on BOTH sides (they were clamped below only); small systems run the
    2-launch k_cg_turn_sym, whose loads are the same."""
    case = synthetic.poisson_block(gx, gy, gz)
    n = case.n_cells
    s = reg.solver(f"tail_{gx}_{gy}_{gz}", cfg(max_iter=12)).set_matrix(case)
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    x0 = np.random.default_rng(n).uniform(-1, 1, n)
    np.testing.assert_array_equal(s.spmv(x0), oracle.spmv(rp, cols, vals, x0))
    b = oracle.spmv(rp, cols, vals, synthetic.x_star(np.arange(n), n))
    x, perf = s.solve(b, np.zeros_like(b))
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    with blocked(oracle, chunk_rows):
        ref = oracle.cg(A, b, np.zeros_like(b), inv, tolerance=0.0, rel_tol=0.0, max_iter=12)
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)


def test_bicgstab_128_nonsymmetric_bit_equal(reg, oracle, chunk_rows):
    case = synthetic.poisson_case(128, symmetric=False)
    s = reg.solver("U128", cfg(solver=capi.SOLVER_BICGSTAB)).set_matrix(case)
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    d_rp, d_cols, _, d_vals = s.local_matrix()
    np.testing.assert_array_equal(d_cols, cols)
    np.testing.assert_array_equal(d_vals, vals)
    b = oracle.spmv(rp, cols, vals, synthetic.x_star(case.global_index, case.global_n))
    x, perf = s.solve(b, np.zeros_like(b))
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=TURNS)
    with blocked(oracle, chunk_rows):
        ref = oracle.bicgstab(A, b, np.zeros_like(b), inv, **kw)
    assert perf.n_iterations == ref.n_iterations // 2                  # GKOBiCGStab.H:114
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x)
    assert perf.norm_factor == ref.norm_factor
    seq = oracle.bicgstab(A, b, np.zeros_like(b), inv, **kw)
    hist = s.history()
    dev = rel_dev(hist, seq.history)
    print(f"128^3 BiCGStab + BJ: max rel deviation from the sequential order over {dev.size} checks {dev.max():.2e}, "
          f"first 5 {dev[:5].max():.2e}, first 12 {dev[:12].max():.2e}")
    # On this non-symmetric system BiCGStab amplifies the rounding difference of two summation orders by about an
    # order of magnitude per few turns while the residual has hardly moved -- a property of the recurrences, the
    # oracle's two orders show it among themselves on the CPU (32^3: 5.7e-8, 64^3: 1.5e-5, 96^3: 1.9e-6 within 30
    # turns): only the leading checks can be held to north_star's 1e-12
    assert dev[:5].max() <= 1e-12 and dev[:12].max() <= 1e-10 and dev.max() <= 1e-4


# ------------------------------------------------------------------------------------------ (d)

def test_gmres30_184_shuffled_first_cycle_bit_equal(reg, oracle, chunk_rows):
    case = synthetic.renumber_case(synthetic.poisson_case(184), 65536)          # 6,229,504 rows
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=31)                          # one restart cycle + its check
    s = reg.solver("c4", cfg(solver=capi.SOLVER_GMRES, krylov_dim=30, max_iter=31)).set_matrix(case)
    new_id = s.renumbering()
    assert new_id is not None                                                   # `renumber auto` took the RCM numbering
    A, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    d_rp, d_cols, _, d_vals = s.local_matrix()
    np.testing.assert_array_equal(d_rp, rp)
    np.testing.assert_array_equal(d_cols, cols)
    np.testing.assert_array_equal(d_vals, vals)
    xs = synthetic.x_star(case.global_index, case.global_n)
    b = oracle.spmv(rp, cols, vals, to_new(xs, new_id))[new_id]                 # caller's order
    x, perf = s.solve(b, np.zeros_like(b))
    P = oracle.Precond(rp, cols, vals, 1)
    with blocked(oracle, chunk_rows):
        ref = oracle.gmres(A, to_new(b, new_id), np.zeros_like(b), P, krylov_dim=30, **kw)
    assert perf.n_iterations == ref.n_iterations
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x[new_id])
    assert perf.norm_factor == ref.norm_factor
    hist = s.history()
    assert hist[31] < hist[30] == hist[1]                                       # the restart moved the criterion's residual


# ------------------------------------------------------------------------------------------ (e)

def test_gtest_init_local_sparsity_through_the_device(reg, golden):
    """unitTests/test_HostMatrix.C:70-107 (+ the two SURVEY 10.2/10.3 runs of the reference function): rows, cols and
    permute as the DEVICE set-up kernels build them."""
    for key in ("init_local_sparsity", "init_local_sparsity_asym", "init_local_sparsity_box2"):
        g = golden[key]
        n, F = g["nrows"], len(g["upper"])
        sym = g["is_symmetric"]
        rng = np.random.default_rng(F)
        case = synthetic.LduCase(n, np.array(g["lower"], np.int32), np.array(g["upper"], np.int32),
                                 rng.uniform(4, 5, n), rng.uniform(-1, 0, F), None if sym else rng.uniform(-1, 0, F))
        s = reg.solver("kat_" + key, cfg()).set_matrix(case)
        assert s.get_property("patternBuiltOnDevice") == 1.0
        rp, cols, mp, vals = s.local_matrix()
        rows = np.repeat(np.arange(n), np.diff(rp))
        assert rows.tolist() == g["rows"]
        assert cols.tolist() == g["cols"]
        assert mp.tolist() == g["permute"]
        src = np.concatenate([case.upper] + ([] if sym else [case.lower]) + [case.diag])
        np.testing.assert_array_equal(vals, src[np.array(g["permute"])])


def test_gtest_symmetric_update_through_the_device(reg, golden):
    """unitTests/test_HostMatrix.C:8-38.  The gtest's permute vector is that of a 5-cell mesh whose faces are NOT in
    upper-triangular order: (0,1) (1,2) (0,3) (2,3) (1,4) (3,4) -- fed through set_matrix, the device must build
    exactly this ldu_mapping and gather exactly the expected coefficients."""
    g = golden["symmetric_update"]
    lower = np.array([0, 1, 0, 2, 1, 3], np.int32)
    upper = np.array([1, 2, 3, 3, 4, 4], np.int32)
    case = synthetic.LduCase(5, lower, upper, np.array(g["diag"], float), np.array(g["upper"], float), None)
    s = reg.solver("kat_sym_update", cfg()).set_matrix(case)
    rp, cols, mp, vals = s.local_matrix()
    assert mp.tolist() == g["permute"]
    assert vals.tolist() == [float(v) for v in g["expected"]]
    # the same through the reorderOnHost branch (symmetric_update proper: `scale` is ignored)
    s2 = reg.solver("kat_sym_update_host", cfg(reorder_on_host=1, scaling=-1.0)).set_matrix(case)
    assert s2.local_matrix()[3].tolist() == [float(v) for v in g["expected"]]


def test_gtest_non_symmetric_update_through_the_device(reg, golden):
    """unitTests/test_HostMatrix.C:40-68.  Its permute vector belongs to the addressing (0,1) (0,2) (1,3) (1,3) (2,4)
    (3,4) -- a face pair listed twice, which no mesh has but the conversion is defined for (ties ordered by source
    slot, as the reference's tuple sort orders them)."""
    g = golden["non_symmetric_update"]
    lower = np.array([0, 0, 1, 1, 2, 3], np.int32)
    upper = np.array([1, 2, 3, 3, 4, 4], np.int32)
    case = synthetic.LduCase(5, lower, upper, np.array(g["diag"], float), np.array(g["upper"], float),
                             np.array(g["lower"], float))
    s = reg.solver("kat_asym_update", cfg(solver=capi.SOLVER_BICGSTAB)).set_matrix(case)
    rp, cols, mp, vals = s.local_matrix()
    assert mp.tolist() == g["permute"]
    assert vals.tolist() == [float(v) for v in g["expected"]]


# ------------------------------------------------------------------------------------------ (f)

def _config2_mesh(which):
    import dataclasses
    if which == "shuffled128":
        return synthetic.renumber_case(synthetic.poisson_case(128, symmetric=False), 65536)      # 2,097,152 rows
    case = synthetic.multi_block_case([60, 90, 40], 104, 104)                                     # 2,055,040 rows
    return dataclasses.replace(case, upper=np.full(case.n_faces, -0.9), lower=np.full(case.n_faces, -1.1))


@pytest.mark.parametrize("which", ["shuffled128", "blocks3"])
@pytest.mark.parametrize("pc,isai", [(capi.PRECOND_ISAI, "spd"), (capi.PRECOND_GISAI, "general")], ids=["ISAI", "GISAI"])
def test_config2_bicgstab_isai_at_size_bit_equal(reg, oracle, chunk_rows, which, pc, isai):
    """configs[2]: GKOBiCGStab + ISAI / GISAI on ~2 M unstructured cells, 10 turns (Preconditioner/Preconditioner.H:225-241,
    Solver/BiCGStab/GKOBiCGStab.H:49-67)."""
    turns = 10
    case = _config2_mesh(which)
    kw = dict(tolerance=0.0, rel_tol=0.0, max_iter=turns)
    s = reg.solver(f"U_{which}_{isai}", cfg(solver=capi.SOLVER_BICGSTAB, preconditioner=pc, max_iter=turns)).set_matrix(case)
    new_id = s.renumbering()
    assert (new_id is not None) == (which == "shuffled128")
    if new_id is None:
        new_id = np.arange(case.n_cells, dtype=np.int32)
    A, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    d_rp, d_cols, _, d_vals = s.local_matrix()
    np.testing.assert_array_equal(d_rp, rp)
    np.testing.assert_array_equal(d_cols, cols)
    np.testing.assert_array_equal(d_vals, vals)
    xs = synthetic.x_star(case.global_index, case.global_n)
    b = oracle.spmv(rp, cols, vals, to_new(xs, new_id))[new_id]                 # caller's order
    x, perf = s.solve(b, np.zeros_like(b))
    # W runs on the compressed layout in every one of these cases; on the renumbered copy ISAI(spd)'s triangle is the
    # CALLER's (rows of 1 .. 7 entries side by side), which qualifies through the length sort inside the windows
    assert s.get_property("isaiWCompressed") == 1.0
    if which == "shuffled128" and isai == "spd":
        assert s.get_property("isaiWSorted") == 1.0 and s.get_property("isaiWtCompressed") == 1.0
    P = oracle_precond_renumbered(oracle, case, rp, cols, vals, new_id, isai=isai)
    with blocked(oracle, chunk_rows):
        ref = oracle.bicgstab(A, to_new(b, new_id), np.zeros_like(b), P, **kw)
    assert perf.n_iterations == ref.n_iterations // 2                  # GKOBiCGStab.H:114
    np.testing.assert_array_equal(s.history(), ref.history)
    np.testing.assert_array_equal(x, ref.x[new_id])
    assert perf.norm_factor == ref.norm_factor
    assert np.isfinite(s.history()).all() and s.history().size == 2 * turns + 1
