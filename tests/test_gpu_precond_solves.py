"""Whole single-rank solves with IC, ILU, IRILU and Multigrid against the oracle, bit for bit.

The apply z = M^-1 r of these kinds is pinned by test_gpu_incomplete_factor.py / test_gpu_multigrid.py, the Krylov loops
by the parity tests with the kinds the oracle's C loops apply themselves.  Here the two meet: the oracle's loop, in the
device's reduction tree, with the kind's NumPy reference called back as its preconditioner (tests/precond_cases.py) -- so
that the gate of the kind's launches past the stop, the rho = r.z partials fused behind the apply, the vectors carried
through a renumbering and the kind's launches inside every turn shape all show in history, x and the counts.  The
references' own soundness (they stop by the tolerance, after 10 checks or more, at the solution) is
test_oracle_precond_callback.py."""
import numpy as np
import pytest

from ogl_amd import capi
import precond_cases as pc
import test_gpu_multigrid as mgmod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def device_solve(reg, field, name, kind, solver, props=(), **kw):
    """(solver object, x, perf, history) of one device solve of a named system from a zero guess."""
    case, b = pc.system(name)[:2]
    base = dict(solver=pc.SOLVER_IDS[solver], preconditioner=pc.KIND_IDS[kind], tolerance=pc.TOL, rel_tol=0.0,
                max_iter=pc.MAX_ITER, export_res=1, adapt_min_iter=0, renumber=capi.RENUMBER_OFF,
                krylov_dim=pc.KRYLOV_DIM, update_init_guess=1)  # (a field solved again starts from the zero guess again)
    base.update(kw)
    s = reg.solver(field, capi.default_config(**base))
    if kind == "MG":
        s.set_multigrid(**pc.MG_DEFAULTS)
    for key, value in props:
        s.set_property(key, value)
    s.set_matrix(case)
    x, perf = s.solve(b, np.zeros_like(b))
    return s, x, perf, s.history()


def assert_is_the_oracles(got, ref, solver):
    s, x, perf, hist = got
    np.testing.assert_array_equal(hist, ref.history)
    np.testing.assert_array_equal(x, ref.x)
    # (the criterion counts GKOBiCGStab's half steps, the solver reports whole ones: as tests/dist_worker.py)
    assert perf.n_iterations == (ref.n_iterations // 2 if solver == "bicgstab" else ref.n_iterations)
    assert perf.n_norm_evals == ref.n_evals
    assert perf.initial_residual == ref.initial_residual and perf.final_residual == ref.final_residual


def shape_of(s):
    return {k: s.get_property(k) for k in ("fusedFinalizersInUse", "leadFinalizersInUse", "fusedTurnInUse")}


# What krylov_plan selects for a kind that materialises z, on a single rank below 48 chunks: GKOCG keeps its finalisers as
# launches of their own (the fused turn has no place for the kind's launches), GKOBiCGStab and GKOGMRES fold them.
FOLDED = {"cg": 0.0, "bicgstab": 1.0, "gmres": 1.0}


@pytest.mark.parametrize("name,kind,solver", pc.MATRIX, ids=lambda v: str(v))
def test_default_turn(reg, name, kind, solver):
    got = device_solve(reg, f"ps_{name}_{kind}_{solver}", name, kind, solver)
    assert shape_of(got[0]) == dict(fusedFinalizersInUse=FOLDED[solver], leadFinalizersInUse=0.0, fusedTurnInUse=0.0)
    assert_is_the_oracles(got, pc.reference(name, kind, solver), solver)


@pytest.mark.parametrize("name,kind,solver,prop", [
    ("asym", "ILU", "bicgstab", "fusedFinalizers"), ("asym", "MG", "bicgstab", "fusedFinalizers"),
    ("sym", "MG", "gmres", "fusedFinalizers"), ("asym", "IRILU", "gmres", "fusedFinalizers"),
    ("asym", "ILU", "bicgstab", "bicgFold"), ("sym", "MG", "bicgstab", "bicgFold"), ("sym", "IC", "bicgstab", "bicgFold"),
    ("sym", "IC", "gmres", "gmresFold"), ("asym", "MG", "gmres", "gmresFold"), ("asym", "IRILU", "gmres", "gmresFold"),
], ids=lambda v: str(v))
def test_unfolded_turn(reg, name, kind, solver, prop):
    """The same solves with the finalisers as launches of their own (properties fusedFinalizers | bicgFold | gmresFold 0):
    the kind's launches sit between other kernels, the bits stay."""
    got = device_solve(reg, f"ps_{prop}_{name}_{kind}_{solver}", name, kind, solver, props=((prop, 0.0),))
    assert shape_of(got[0]) == dict(fusedFinalizersInUse=0.0, leadFinalizersInUse=0.0, fusedTurnInUse=0.0)
    assert_is_the_oracles(got, pc.reference(name, kind, solver), solver)


STOPS = [("sym", "IC", "cg"), ("asym", "ILU", "bicgstab"), ("sym", "MG", "cg"), ("sym", "MG", "gmres")]


@pytest.mark.parametrize("max_iter", [1, 2, 16, 17])
@pytest.mark.parametrize("name,kind,solver", STOPS, ids=lambda v: str(v))
def test_stop_at_a_fixed_turn(reg, name, kind, solver, max_iter):
    """tolerance 0: the solve ends at max_iter, on both sides of the first batch of enqueued turns.  Every launch of the
    kind past the stop must be a no-op: x is the oracle's, not one turn further."""
    crit = dict(tolerance=0.0, max_iter=max_iter)
    got = device_solve(reg, f"ps_stop_{name}_{kind}_{solver}", name, kind, solver, **crit)
    ref = pc.reference(name, kind, solver, **crit)
    assert ref.n_iterations == (2 * max_iter if solver == "bicgstab" else max_iter) + 1
    assert_is_the_oracles(got, ref, solver)


def test_gmres_stops_inside_the_third_cycle(reg):
    crit = dict(tolerance=0.0, max_iter=12, krylov_dim=5)
    got = device_solve(reg, "ps_stop_gmres5", "sym", "MG", "gmres", **crit)
    assert_is_the_oracles(got, pc.reference("sym", "MG", "gmres", **crit), "gmres")


@pytest.mark.parametrize("name,kind,solver", [("chunks48", "IC", "cg"), ("chunks48", "MG", "cg"),
                                              ("chunks48_asym", "ILU", "bicgstab")], ids=lambda v: str(v))
def test_leader_finalisation(reg, name, kind, solver):
    """48 chunks, the smallest system krylov_plan gives the leader turn (fusedFinMaxChunks 1 takes the folded
    single-workgroup finalisers away): the kind's launches between step_2r and the next turn's check, 12 turns."""
    crit = dict(tolerance=0.0, max_iter=12)
    got = device_solve(reg, f"ps_lead_{kind}", name, kind, solver, props=(("fusedFinMaxChunks", 1.0),), **crit)
    assert shape_of(got[0]) == dict(fusedFinalizersInUse=0.0, leadFinalizersInUse=1.0, fusedTurnInUse=0.0)
    assert_is_the_oracles(got, pc.reference(name, kind, solver, **crit), solver)


@pytest.mark.parametrize("graph", [1.0, 0.0])
def test_hip_graph_on_and_off(reg, graph):
    """Property hipGraph either way (a turn with a materialised z is not captured: krylov_loop): the oracle's bits."""
    got = device_solve(reg, f"ps_graph_{graph}", "sym", "MG", "cg", props=(("hipGraph", graph),))
    assert_is_the_oracles(got, pc.reference("sym", "MG", "cg"), "cg")


@pytest.mark.parametrize("layout", sorted(mgmod.LAYOUTS))
def test_multigrid_on_every_in_loop_layout(reg, layout):
    kw, (lay, half) = mgmod.LAYOUTS[layout]
    got = device_solve(reg, "ps_lay_" + layout, "sym", "MG", "cg", props=(("streamAboveBytes", 0.0),), **kw)
    s = got[0]
    assert s.get_property("spmvLayout") == lay and s.get_property("symmetricHalf") == half
    assert s.get_property("spmvStream") == 1.0
    assert_is_the_oracles(got, pc.reference("sym", "MG", "cg"), "cg")


@pytest.mark.parametrize("kind", ["IC", "MG"])
def test_renumbered_device_copy(reg, kind):
    """renumber on: the oracle solves the system permuted by the numbering the library reports; the factor and the
    hierarchy stay those of the caller's numbering, r and z are carried through the permutation around them."""
    got = device_solve(reg, "ps_renumbered_" + kind, "shuffled14", kind, "cg", renumber=capi.RENUMBER_ON)
    s = got[0]
    new_id = s.renumbering()
    assert new_id is not None and s.get_property("renumbered") == 1.0
    assert not np.array_equal(new_id, np.arange(new_id.size))
    ref = pc.reference("shuffled14", kind, "cg", new_id=new_id)
    pc.check_sound(ref, pc.system("shuffled14")[2])
    assert_is_the_oracles(got, ref, "cg")


@pytest.mark.parametrize("kind", ["IC", "MG"])
def test_irregular_mesh(reg, kind):
    got = device_solve(reg, "ps_voronoi_" + kind, "voronoi", kind, "cg")
    assert_is_the_oracles(got, pc.reference("voronoi", kind, "cg"), "cg")


# ---- negative controls: a comparison that passed against a wrong reference would be worthless ----
class NoLastPostSweep(mgmod.Ref):
    """The V-cycle without the last post-smoothing sweep on every level: deliberately not the contract."""

    def cycle(self, l, b, fine=None):
        A = fine if (l == 0 and fine is not None) else self.A[l]
        if l == self.levels - 1:
            return self.cg(A, b)
        x = mgmod.OMEGA * (b * self.inv_d[l])
        x = self.sweep(l, b, x, A)
        res = b - A.mul(x)
        order, ptr = self.members[l]
        bc = mgmod.seq_sums(ptr[:-1], np.diff(ptr), res[order], init=np.zeros(len(ptr) - 1))
        x = x + self.cycle(l + 1, bc)[self.agg[l]]
        return self.sweep(l, b, x, A)


def first_difference(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(a[:m] != b[:m])
    return int(d[0]) if len(d) else None


def test_a_nudged_omega_shows_in_the_first_three_entries(reg, monkeypatch):
    _, _, _, hist = device_solve(reg, "ps_negative", "sym", "MG", "cg")
    right = pc.precond_ref("sym", "MG")
    monkeypatch.setattr(mgmod, "OMEGA", 0.9 * (1 + 2.0 ** -40))

    def nudged(r):  # (a function of its own: a reference cached under another `apply` than the right one)
        return right.apply(r)
    ref = pc.reference("sym", "MG", "cg", apply=nudged)
    monkeypatch.undo()
    where = first_difference(hist, ref.history)
    assert where is not None and where < 3, where
    np.testing.assert_array_equal(hist, pc.reference("sym", "MG", "cg").history)  # (and the right one still compares equal)


def test_a_missing_post_sweep_shows_at_entry_1(reg, oracle):
    _, _, _, hist = device_solve(reg, "ps_negative", "sym", "MG", "cg")
    wrong = NoLastPostSweep(oracle, *pc.system("sym")[3], **pc.MG_DEFAULTS)
    ref = pc.reference("sym", "MG", "cg", apply=wrong.apply)
    assert hist[0] == ref.history[0]  # (the first check sees r alone)
    assert first_difference(hist, ref.history) == 1
