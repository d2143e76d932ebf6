"""The held-z turn (kernels_krylov.hip, k_cg_step2r1x) in the parts of its work mapping that tests/test_gpu_held_z.py does not
reach: workgroups that own all 20 chunks (11 in registers, LDS slots 0 .. 8), the tagged sums in their second and third
polling round and in rounds that only some lanes take part in, the capacity of the grid itself, the kernel's own copy of
the stopping criterion (rel_tol, min_iter), heldZEarlyX 0, every SpMV kernel that produces the partials of beta, a device
copy in another numbering, the life cycle of a handle and the breakdown branch beta == 0.

Every comparison is bit for bit: heldZ 1 against heldZ 0 (the three-launch leader turn) and against the oracle run in the
device's reduction tree.  Every run asserts heldZInUse, heldZGridInUse (whether heldZGrid was honoured or clipped by the
device) and leadFinalizersInUse.  Chunk arithmetic: with G workgroups, workgroup w owns mine = (chunks - w + G - 1) / G
chunks, chunk w + i G in slot i; slots 0 .. 10 are registers, 11 .. 19 LDS slots 0 .. 8.  Lines (poisson_block(rows, 1, 1))
give exact chunk counts and cost the oracle little; boxes where the layout matters.  An oracle run is made once per
(system, preconditioner, start vector, criterion) and shared by the cases that need it."""
import dataclasses
import gc
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_matrix, oracle_matrix_renumbered, to_new

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soak_worker  # noqa: E402

CHUNK = 512
PER_WG = 20   # chunks a workgroup holds: 11 in registers + 9 in LDS
Out = namedtuple("Out", "x n_iterations history final_residual n_norm_evals")
System = namedtuple("System", "case b A csr inv")


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()
    _systems.clear()
    _refs.clear()


_systems = {}
_refs = {}


def system_of(oracle, key, make):
    if key not in _systems:
        case = make()
        b = synthetic.rhs_for_x_star(case)[0]
        A, csr = oracle_matrix(oracle, case)
        _systems[key] = System(case, b, A, csr, oracle.jacobi_generate_scalar(*csr))
    return _systems[key]


def line(oracle, rows):
    return system_of(oracle, ("line", rows), lambda: synthetic.poisson_block(rows, 1, 1))


def box(oracle, n):
    return system_of(oracle, ("box", n), lambda: synthetic.poisson_case(n))


def reference(oracle, key, sy, precond, x0=None, b=None, **crit):
    """oracle.cg in the device's reduction tree, once per key."""
    key = (key, precond, tuple(sorted(crit.items())))
    if key not in _refs:
        b = sy.b if b is None else b
        with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
            _refs[key] = oracle.cg(sy.A, b, np.zeros_like(b) if x0 is None else x0, sy.inv if precond else None, **crit)
    return _refs[key]


def device_kw(crit):
    kw = dict(crit)
    if "frequency" in kw:
        kw["eval_frequency"] = kw.pop("frequency")
    return kw


def run(reg, name, case, b, held, grid, defer=2.0, early=1.0, props=(), x0=None, expect=None, precond=capi.PRECOND_BJ,
        cfg=None, **crit):
    """One solve on the handle `name`.  held: the property heldZ; expect: what heldZInUse must report (default: held)."""
    c = capi.default_config(solver=capi.SOLVER_CG, export_res=1, adapt_min_iter=0, update_init_guess=1,
                            preconditioner=precond, **(cfg or {}), **device_kw(crit))
    s = reg.solver(name, c)
    for key, v in (("fusedFinMaxChunks", 0.0),  # (the leader turn from 48 chunks on)
                   ("fusedTurnBig", 0.0),       # (its three-launch form: what the held-z turn replaces)
                   ("heldZ", held), ("deferX", defer), ("heldZGrid", float(grid)), ("heldZEarlyX", early), *props):
        s.set_property(key, v)
    s.set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b) if x0 is None else x0)
    on = held if expect is None else expect
    assert s.get_property("heldZInUse") == on
    assert s.get_property("heldZGridInUse") == (float(grid) if on else 0.0)
    assert s.get_property("leadFinalizersInUse") == 1.0 and s.get_property("fusedTurnInUse") == 0.0
    assert s.get_property("deferXInUse") == defer
    return Out(x, perf.n_iterations, s.history().copy(), perf.final_residual, perf.n_norm_evals), s


def assert_same(a, b):
    assert a.n_iterations == b.n_iterations and a.n_norm_evals == b.n_norm_evals
    np.testing.assert_array_equal(a.history, b.history)   # (NaN equals NaN here)
    np.testing.assert_array_equal(a.x, b.x)
    np.testing.assert_array_equal(a.final_residual, b.final_residual)


def assert_oracle(a, ref, new_id=None):
    assert a.n_iterations == ref.n_iterations and a.n_norm_evals == ref.n_evals
    np.testing.assert_array_equal(a.history, ref.history)
    np.testing.assert_array_equal(a.x, ref.x if new_id is None else ref.x[new_id])
    np.testing.assert_array_equal(a.final_residual, ref.final_residual)


def on_off_oracle(reg, oracle, name, key, sy, grid, precond, defer, crit, early=1.0, x0=None, b=None, props=()):
    """heldZ 1 against heldZ 0 against the oracle; returns the held-z run."""
    b = sy.b if b is None else b
    out = {h: run(reg, f"{name}_{h}", sy.case, b, h, grid, defer, early, props=props, x0=x0, precond=precond, **crit)[0]
           for h in (1.0, 0.0)}
    assert_same(out[1.0], out[0.0])
    assert_oracle(out[1.0], reference(oracle, key, sy, precond, x0=x0, b=b, **crit))
    return out[1.0]


def probe_history(oracle, key, sy, precond=capi.PRECOND_BJ, turns=60):
    return reference(oracle, key, sy, precond, tolerance=0.0, rel_tol=0.0, max_iter=turns).history


def probe_tolerance(oracle, key, sy):
    """A tolerance that a run with evalFrequency 3 first meets well inside it: the residual of turn 40 of the probe (the
    histories rise before they fall and are not monotone after, so the stop may lie before turn 40; never at turn 0)."""
    h = probe_history(oracle, key, sy)
    assert h[40] < h[:4].min()
    return float(h[40])


# ---- A, E: fully loaded workgroups on small systems ----
# name -> (system, heldZGrid); what the chunk arithmetic gives is asserted in test_full_load_geometry
FULL = {
    "line640": (lambda o: line(o, 640 * CHUNK), 32),            # all 32 workgroups own 20 chunks, all of them leaders
    "line639+1": (lambda o: line(o, 639 * CHUNK + 1), 32),      # 640 chunks, the last one (LDS slot 8 of workgroup 31) of one row
    "line638+1": (lambda o: line(o, 638 * CHUNK + 1), 32),      # 639 chunks: workgroup 31 owns 19, its last chunk has one row
    "line640-1": (lambda o: line(o, 640 * CHUNK - 1), 32),      # the last thread pair holds one row, in LDS slot 8
    "line660": (lambda o: line(o, 660 * CHUNK), 33),            # workgroup 32: fully loaded and no leader of the sums
    "box84": (lambda o: box(o, 84), 58),                        # 56 workgroups own 20, two own 19; cap 1,160 >= 1,158
}


def owned(chunks, grid):
    return [(chunks - w + grid - 1) // grid if w < chunks else 0 for w in range(grid)]


def test_full_load_geometry():
    """The arithmetic the cases below rest on (no device needed for it, but it belongs to them)."""
    assert owned(640, 32) == [20] * 32
    assert owned(640, 32) == owned(-(-(640 * CHUNK - 1) // CHUNK), 32) and (640 * CHUNK - 1) % CHUNK == CHUNK - 1
    assert owned(-(-(639 * CHUNK + 1) // CHUNK), 32) == [20] * 32 and (639 * CHUNK + 1) % CHUNK == 1
    assert owned(-(-(638 * CHUNK + 1) // CHUNK), 32) == [20] * 31 + [19] and (638 * CHUNK + 1) % CHUNK == 1
    assert owned(660, 33) == [20] * 33
    n84 = -(-84 ** 3 // CHUNK)
    assert n84 == 1158 and owned(n84, 58) == [20] * 56 + [19] * 2 and 58 * PER_WG == 1160
    assert max(owned(n84, 100)) == 12   # (tests/test_gpu_held_z.py: LDS slot 0 only)


@pytest.mark.parametrize("early", [1.0, 0.0], ids=["earlyx1", "earlyx0"])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE], ids=["BJ", "none"])
@pytest.mark.parametrize("which", list(FULL))
def test_full_load_wherever_max_iter_stops(reg, oracle, which, precond, defer, early):
    """LDS slots 0 .. 8 and the prefetch of slots 18 and 19; stops in the first, second and third batch of 16 turns, at
    both ring positions.  heldZEarlyX 0 (the x update of a head that does not defer inside the phase-2 loop) gives the
    bits of heldZEarlyX 1, both being compared with heldZ 0 and the oracle."""
    make, grid = FULL[which]
    sy = make(oracle)
    for max_iter in (16, 17, 33):
        crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
        got = on_off_oracle(reg, oracle, f"full_{which}_{precond}_{defer}_{early}", which, sy, grid, precond, defer, crit, early)
        assert got.n_iterations == max_iter + 1


@pytest.mark.parametrize("early", [1.0, 0.0], ids=["earlyx1", "earlyx0"])
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("which", list(FULL))
def test_full_load_stops_by_tolerance(reg, oracle, which, defer, early):
    """A tolerance that is a value of the history itself, evalFrequency 3: the stop lies inside the run, on a turn where
    x need not be up to date."""
    make, grid = FULL[which]
    sy = make(oracle)
    tol = probe_tolerance(oracle, which, sy)
    crit = dict(tolerance=tol, rel_tol=0.0, max_iter=600, frequency=3)
    got = on_off_oracle(reg, oracle, f"full_tol_{which}_{defer}_{early}", which, sy, grid, capi.PRECOND_BJ, defer, crit, early)
    assert 3 < got.n_iterations < 600


# ---- B: the capacity of the grid itself ----
@pytest.mark.parametrize("grid,chunks,on", [(32, 640, 1.0), (32, 641, 0.0), (31, 600, 0.0), (31, 48, 0.0)],
                         ids=["32x20", "32x20+1", "31-fits", "31-small"])
def test_capacity_through_the_grid(reg, oracle, grid, chunks, on):
    """grid x 20 chunks fit and one more does not, by the grid's own cap (heldZMaxChunks is not set); 31 workgroups are
    fewer than the 2 x 16 leaders of the sums, whatever the size.  Off means the three-launch turn's bits."""
    sy = line(oracle, chunks * CHUNK)
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=17)
    asked = run(reg, f"cap_{grid}_{chunks}_on", sy.case, sy.b, 1.0, grid, expect=on, **crit)[0]
    off = run(reg, f"cap_{grid}_{chunks}_off", sy.case, sy.b, 0.0, grid, **crit)[0]
    assert_same(asked, off)
    assert_oracle(asked, reference(oracle, ("line", chunks), sy, capi.PRECOND_BJ, **crit))


def device_grid():
    """Four workgroups per compute unit: the resident grid of the held-z turn (1,024 on MI355X)."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("extra,on", [(0, 1.0), (1, 0.0)], ids=["full", "full+1"])
def test_capacity_of_the_device(oracle, extra, on):
    """device grid x 20 chunks on a line (20,480 x 512 = 10,485,760 rows on MI355X): every workgroup of the full grid is
    fully loaded, the tagged sums take five polling rounds.  One row more is one chunk more: off.  Four turns.  The oracle
    follows the first (about 0.1 s per turn on a line); the second is compared with heldZ 0 alone -- the same kernels
    as the 641-chunk case above, at a size that only the gate makes special."""
    grid = device_grid()
    rows = grid * PER_WG * CHUNK + extra
    case = synthetic.poisson_block(rows, 1, 1)
    b = synthetic.rhs_for_x_star(case)[0]
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=4)
    r = capi.Registry()
    try:
        asked = run(r, "dev_cap_on", case, b, 1.0, grid, expect=on, **crit)[0]
        off = run(r, "dev_cap_off", case, b, 0.0, grid, **crit)[0]
    finally:
        r.close()
    assert_same(asked, off)
    if not extra:
        A, csr = oracle_matrix(oracle, case)
        with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
            ref = oracle.cg(A, b, np.zeros_like(b), oracle.jacobi_generate_scalar(*csr), **crit)
        assert_oracle(asked, ref)
    gc.collect()


# ---- C: the polling rounds of the tagged sums ----
# a lane of a leader takes partials v, v + 1024, v + 2048, v + 3072 in its first round, v + 4096 .. in its second
@pytest.mark.parametrize("max_iter", [16, 17])
@pytest.mark.parametrize("grid,chunks", [(1024, 2048), (1024, 2049), (1024, 3073), (1024, 4096), (1024, 4097), (1024, 8193),
                                         (256, 4097), (256, 5120)])
def test_polling_rounds(reg, oracle, grid, chunks, max_iter):
    """2,048 / 2,049 and 3,073: two, three and four partials of a round present in some lanes only; 4,096 / 4,097: one lane
    of one leader enters a second round; 8,193: a third.  256 workgroups at 4,097 and 5,120 chunks own 16 .. 20 chunks each:
    LDS-held z and a second round in one run (and partials polled in another order than they are produced)."""
    grid = min(grid, device_grid())
    sy = line(oracle, chunks * CHUNK)
    assert max(owned(chunks, grid)) <= PER_WG
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    on_off_oracle(reg, oracle, f"poll_{grid}_{chunks}", ("line", chunks), sy, grid, capi.PRECOND_BJ, 2.0, crit)


@pytest.mark.parametrize("grid,chunks", [(1024, 4097), (256, 5120)])
def test_polling_rounds_stop_by_tolerance(reg, oracle, grid, chunks):
    grid = min(grid, device_grid())
    sy = line(oracle, chunks * CHUNK)
    tol = probe_tolerance(oracle, ("line", chunks), sy)
    crit = dict(tolerance=tol, rel_tol=0.0, max_iter=600, frequency=3)
    got = on_off_oracle(reg, oracle, f"poll_tol_{grid}_{chunks}", ("line", chunks), sy, grid, capi.PRECOND_BJ, 2.0, crit)
    assert 3 < got.n_iterations < 600


# ---- D: the criterion as the kernel writes it out ----
def stops_at(h, tolerance=0.0, rel_tol=0.0, min_iter=0, max_iter=600, frequency=1):
    """The turn at which the criterion stops a run whose residuals are h (StoppingCriterion semantics: no verdict below
    min_iter nor off the frequency).  Used only to state where a case is MEANT to stop; the bits come from the oracle."""
    for k in range(len(h)):
        if (0 < k < min_iter) or k % frequency:
            continue
        if k >= max_iter or h[k] < tolerance or (rel_tol > 0 and h[k] < rel_tol * h[0]):
            return k
    raise AssertionError("no stop inside the probe")


def criteria(h):
    """name -> (criterion, the turn it is built to stop at).  h: the history of 60 turns with tolerance 0.  It is not
    monotone, so every bound lies half way between a record low h[k] and the lowest value before it: first met at turn k."""
    def first_met_at(k):
        assert h[k] < h[:k].min()
        return 0.5 * float(h[k] + h[:k].min())

    tol7, tol14, tol21, tol28 = (first_met_at(k) for k in (7, 14, 21, 28))
    assert h[0] == 1.0   # (so that rel_tol * initial residual is the bound itself)
    assert max(h[18], h[20], h[21]) < tol7   # (met again at the turns min_iter lets the criterion look at)
    return {
        "rel_tol": (dict(tolerance=0.0, rel_tol=tol21, max_iter=600), 21),
        "tolerance-before-rel_tol": (dict(tolerance=tol14, rel_tol=tol28, max_iter=600), 14),
        "rel_tol-before-tolerance": (dict(tolerance=tol28, rel_tol=tol14, max_iter=600), 14),
        # met at 14, which the criterion does not look at; 15 and 18 lie above the bound again
        "rel_tol-freq3": (dict(tolerance=0.0, rel_tol=tol14, max_iter=600, frequency=3), 21),
        # the tolerance is met at turn 7, the criterion may not look before min_iter: it stops AT min_iter when that is a
        # turn it evaluates (iter < min_iter skips, iter == min_iter does not), else at the next multiple
        "min_iter20-freq1": (dict(tolerance=tol7, rel_tol=0.0, min_iter=20, max_iter=600), 20),
        "min_iter21-freq3": (dict(tolerance=tol7, rel_tol=0.0, min_iter=21, max_iter=600, frequency=3), 21),
        "min_iter20-freq3": (dict(tolerance=tol7, rel_tol=0.0, min_iter=20, max_iter=600, frequency=3), 21),
        "min_iter18-rel_tol-freq3": (dict(tolerance=0.0, rel_tol=tol7, min_iter=18, max_iter=600, frequency=3), 18),
        # max_iter 17 is no multiple of 3: the first evaluated turn at or after it is 18
        "max_iter17-freq3": (dict(tolerance=0.0, rel_tol=0.0, max_iter=17, frequency=3), 18),
        "max_iter17-freq3-min_iter19": (dict(tolerance=0.0, rel_tol=0.0, min_iter=19, max_iter=17, frequency=3), 21),
    }


CRITERIA = ["rel_tol", "tolerance-before-rel_tol", "rel_tol-before-tolerance", "rel_tol-freq3", "min_iter20-freq1",
            "min_iter21-freq3", "min_iter20-freq3", "min_iter18-rel_tol-freq3", "max_iter17-freq3",
            "max_iter17-freq3-min_iter19"]


@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("which", CRITERIA)
def test_criterion_inside_the_kernel(reg, oracle, which, defer):
    """rel_tol, min_iter and their combinations with evalFrequency on a fully loaded grid (640 chunks, 32 workgroups):
    iteration count, n_norm_evals, history and x as the three-launch turn's and the oracle's.  The turn each criterion is
    built to stop at is asserted too, so a case that stops elsewhere than intended is seen."""
    sy = line(oracle, 640 * CHUNK)
    h = probe_history(oracle, "line640", sy)
    crit, turn = criteria(h)[which]
    assert stops_at(h, **crit) == turn
    got = on_off_oracle(reg, oracle, f"crit_{defer}", "line640", sy, 32, capi.PRECOND_BJ, defer, crit)
    assert got.n_iterations == turn + 1


# ---- F: every producer of the partials of beta ----
LAYOUT_N = 60     # 216,000 rows = 422 chunks: 32 workgroups own 13 or 14 chunks (LDS slots 0 .. 2)
# name -> (config, (spmvLayout, symmetricHalf, symmetricHalfPerChunk))
LAYOUTS = {
    "sym": (dict(), (2.0, 1.0, 0.0)),
    "sell": (dict(symmetric_half=0), (2.0, 0.0, 0.0)),
    "csr": (dict(compress_indices=0), (0.0, 0.0, 0.0)),
    "ell": (dict(matrix_format=capi.FORMAT_ELL), (1.0, None, None)),
    "symx": (dict(compress_indices=2), (2.0, 1.0, 1.0)),
}


def layout_system(oracle, name):
    if name == "symx":   # three blocks glued along x: banded block by block, the per-chunk half storage
        return system_of(oracle, "blocks3", lambda: synthetic.multi_block_case([20, 30, 10], LAYOUT_N, LAYOUT_N))
    return box(oracle, LAYOUT_N)


@pytest.mark.parametrize("precond", [capi.PRECOND_BJ, capi.PRECOND_NONE], ids=["BJ", "none"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_spmv_layout_feeds_the_turn(reg, oracle, name, precond):
    """The SpMV in front of the resident kernel writes the partials of p.q that its leaders add: k_spmv_sym, the compressed
    full storage, CSR-stream, ELL and the per-chunk half storage, each in its streaming instantiation (streamAboveBytes 0:
    what the default gate asks for).  The layout properties prove which kernel ran."""
    cfg, (layout, half, per_chunk) = LAYOUTS[name]
    sy = layout_system(oracle, name)
    key = "blocks3" if name == "symx" else ("box", LAYOUT_N)
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=33)
    out = {}
    for h in (1.0, 0.0):
        out[h], s = run(reg, f"layout_{name}_{h}", sy.case, sy.b, h, 32, precond=precond, cfg=cfg,
                        props=(("streamAboveBytes", 0.0),), **crit)
        assert s.get_property("spmvLayout") == layout and s.get_property("spmvStream") == 1.0
        assert half is None or s.get_property("symmetricHalf") == half
        assert per_chunk is None or s.get_property("symmetricHalfPerChunk") == per_chunk
        assert s.renumbering() is None
    assert_same(out[1.0], out[0.0])
    assert_oracle(out[1.0], reference(oracle, key, sy, precond, **crit))


@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_renumbered_device_copy(reg, oracle, defer):
    """renumber on over a box shuffled in windows of 65,536 cells: b and x cross the boundary through the permute kernels,
    the resident kernel writes x in device order.  The oracle gets the permutation the library reports."""
    case = synthetic.renumber_case(synthetic.poisson_case(LAYOUT_N), 65536)
    b = synthetic.apply_case(case, synthetic.x_star(case.global_index, case.global_n))
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=33)
    out = {}
    for h in (1.0, 0.0):
        out[h], s = run(reg, f"renum_{defer}_{h}", case, b, h, 32, defer, cfg=dict(renumber=capi.RENUMBER_ON),
                        props=(("streamAboveBytes", 0.0),), **crit)
        assert s.get_property("renumbered") == 1.0 and s.get_property("spmvStream") == 1.0
        new_id = s.renumbering()
        assert new_id is not None and not np.array_equal(new_id, np.arange(case.n_cells))
    assert_same(out[1.0], out[0.0])
    A, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
        ref = oracle.cg(A, to_new(b, new_id), np.zeros_like(b), oracle.jacobi_generate_scalar(rp, cols, vals), **crit)
    assert_oracle(out[1.0], ref, new_id)


# ---- G: life cycle ----
@pytest.mark.parametrize("defer", [0.0, 2.0])
def test_start_vector_that_has_not_converged(reg, oracle, defer):
    sy = box(oracle, 84)
    xs = synthetic.x_star(sy.case.global_index, sy.case.global_n)
    x0 = xs + 1e-3 * np.random.default_rng(84).uniform(-1, 1, xs.size)
    crit = dict(tolerance=1e-7, rel_tol=0.0, max_iter=600)
    got = on_off_oracle(reg, oracle, f"start_{defer}", ("box84", "x0"), sy, 58, capi.PRECOND_BJ, defer, crit, x0=x0)
    assert 3 < got.n_iterations < 600


def test_new_coefficients_between_solves(reg, oracle):
    """Three solves on one handle, the coefficients rescaled in between (the pattern stays: values only), against three
    fresh handles with the turn on and off and against the oracle."""
    base = box(oracle, 84)
    crit = dict(tolerance=1e-6, rel_tol=0.0, max_iter=600)
    for i, scale in enumerate((1.0, 1.25, 1.0625)):
        case = dataclasses.replace(base.case, diag=base.case.diag * scale)
        b = synthetic.rhs_for_x_star(case)[0]
        A, csr = oracle_matrix(oracle, case)
        sy = System(case, b, A, csr, oracle.jacobi_generate_scalar(*csr))
        same = run(reg, "coeff_same_handle", case, b, 1.0, 58, **crit)[0]
        assert_same(same, run(reg, f"coeff_fresh_on_{i}", case, b, 1.0, 58, **crit)[0])
        assert_same(same, run(reg, f"coeff_fresh_off_{i}", case, b, 0.0, 58, **crit)[0])
        assert_oracle(same, reference(oracle, ("box84", "scaled", scale), sy, capi.PRECOND_BJ, **crit))
        assert 3 < same.n_iterations < 600


@pytest.mark.parametrize("graph", [0.0, 1.0])
def test_a_larger_pattern_on_the_same_handle(reg, oracle, graph):
    """set_matrix of 104^3 (2,197 chunks) on a handle that has solved 84^3 (1,158 chunks) on a smaller grid: the box of
    tagged partials grows, the census runs again for the larger grid, and a captured graph is keyed anew."""
    small, large = box(oracle, 84), box(oracle, 104)
    assert -(-large.case.n_cells // CHUNK) == 2197 and max(owned(2197, 128)) == 18
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=40)
    name = f"regrow_{graph}"
    first, s = run(reg, name, small.case, small.b, 1.0, 100, props=(("hipGraph", graph), ("hipGraphCaptures", 0.0)), **crit)
    captures = s.get_property("hipGraphCaptures")
    assert (captures >= 1.0) == (graph == 1.0)
    second, s = run(reg, name, large.case, large.b, 1.0, 128, props=(("hipGraph", graph),), **crit)
    assert (s.get_property("hipGraphCaptures") > captures) == (graph == 1.0)
    for h in (1.0, 0.0):
        assert_same(second, run(reg, f"regrow_fresh_{graph}_{h}", large.case, large.b, h, 128, props=(("hipGraph", graph),),
                                **crit)[0])
    assert_oracle(first, reference(oracle, "box84", small, capi.PRECOND_BJ, **crit))
    assert_oracle(second, reference(oracle, "box104", large, capi.PRECOND_BJ, **crit))
    # ... and back to the small one: the box is reused as it is
    assert_same(first, run(reg, name, small.case, small.b, 1.0, 100, props=(("hipGraph", graph),), **crit)[0])


def test_tags_of_an_earlier_solve_do_not_survive(reg, oracle):
    """The box of tagged partials is cleared with every solve.  If it were not, every word would keep the tag of the last
    turn of the solve before, and the turn of the same number in the next solve would find it `arrived`: wrong if a
    leader polled before the producer had overwritten it.  A solve that stops after K turns, then one with another
    right-hand side that passes turn K, for ten values of K on one handle: the second is the oracle's every time.
    609 chunks on 32 workgroups put the producer as far behind the leader as the mapping allows: workgroup 0 owns 20
    chunks, the others 19, and chunk 608 is polled by leaders 9 and 25, which are through with their own chunks one
    chunk before workgroup 0 publishes it.  (Even so the producer wins that race on MI355X: a library without the
    clearing passed this test, DESIGN.md section 4.2.  It pins the life cycle; it does not prove the memset.)"""
    sy = line(oracle, 609 * CHUNK)
    assert owned(609, 32) == [20] + [19] * 31 and 608 // 64 == 9
    b2 = np.random.default_rng(609).uniform(-1, 1, sy.case.n_cells)
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=40)
    ref = reference(oracle, ("line609", "b2"), sy, capi.PRECOND_BJ, b=b2, **crit)
    for defer in (2.0, 0.0):
        for k in range(4, 14):
            run(reg, f"stale_{defer}", sy.case, sy.b, 1.0, 32, defer, tolerance=0.0, rel_tol=0.0, max_iter=k)
            assert_oracle(run(reg, f"stale_{defer}", sy.case, b2, 1.0, 32, defer, **crit)[0], ref)


def test_time_steps_with_the_turn_on_leave_nothing_behind():
    """40 time steps (new coefficients, set_matrix, solve) on 30^3 with the turn forced on: the ledger stands still between
    steps 10 and 40, and the turn allocates no more often than the three-launch turn does (the census, which allocates
    its two words, runs once per handle)."""
    case = synthetic.poisson_case(30)
    b = synthetic.rhs_for_x_star(case)[0]
    crit = dict(tolerance=1e-6, rel_tol=0.0, max_iter=400)
    gc.collect()
    calls = {}
    for held in (1.0, 0.0):
        r = capi.Registry()
        marks = {}
        for step in range(41):
            case.diag[:] = case.diag * (1.0 + 1e-9)
            out = run(r, "step", case, b, held, 32, **crit)[0]
            assert 1 <= out.n_iterations < 400
            if step in (10, 40):
                marks[step] = capi.memory_ledger().as_dict()
        r.close()
        for k in soak_worker.LEDGER_EXACT:
            assert marks[40][k] == marks[10][k], (held, k, marks)
        assert marks[40]["unknown_frees"] == 0
        calls[held] = marks[40]["device_alloc_calls"] - marks[10]["device_alloc_calls"]
    assert calls[1.0] == calls[0.0], calls


# ---- H: breakdown ----
@pytest.mark.parametrize("defer", [0.0, 2.0])
@pytest.mark.parametrize("max_iter", [3, 4])
def test_breakdown_with_an_exact_start_vector(reg, oracle, max_iter, defer):
    """x0 = x* and b = A x* by the oracle's row loop.  The residual's row loop (b - a_0 x_0 - a_1 x_1 ...) adds in another
    order than b's, so the coefficients are dyadic (diagonal 2.5, off-diagonals -1) and x* holds small integers: every
    product and sum is exact, r = 0 exactly, p.q = 0, beta == 0.  No term of x of its own, rho / prev_rho taken as 0,
    t_ring left alone: the resident kernel, the three-launch turn and the oracle must leave the same x, history and
    scalars."""
    def dyadic():
        case = synthetic.poisson_block(640 * CHUNK, 1, 1)
        return dataclasses.replace(case, diag=np.full(case.n_cells, 2.5))

    sy = system_of(oracle, "line640-dyadic", dyadic)
    xs = np.random.default_rng(640).integers(-8, 9, sy.case.n_cells).astype(np.float64)
    b = oracle.spmv(*sy.csr, xs)
    crit = dict(tolerance=0.0, rel_tol=0.0, max_iter=max_iter)
    got = on_off_oracle(reg, oracle, f"breakdown_{defer}", "line640-dyadic", sy, 32, capi.PRECOND_BJ, defer, crit, x0=xs, b=b)
    assert got.n_iterations == max_iter + 1
    np.testing.assert_array_equal(got.history, np.zeros(max_iter + 1))
    np.testing.assert_array_equal(got.x, xs)
