"""IC, ILU, IRILU (exact, `triangularSolves isai`, `factorSweeps`), Chebyshev and Multigrid on drawn irregular systems
(tests/random_precond_cases.py) against their NumPy references, bit for bit: patterns that are no box, row counts that are
no product of three small numbers, a level per row, two rows, one row.  Per case, so that a failure names the earliest
stage: what the generation reports, z = M^-1 r, then a whole solve from zero (tolerance 1e-12, 12 iterations at most; CG on
the symmetric cases, BiCGStab on the others, GMRES(5) on every third) against the oracle's loop in the device's reduction
tree with the reference called back.  One registry per test and one field per variant: the field meets another pattern,
another size, another solver and another numbering with every case.

The comparisons are the four check_* helpers; tests/test_random_precond_cases.py calls each of them without a device, with
a reference that is wrong in one place, and expects the AssertionError."""
import numpy as np
import pytest

from ogl_amd import capi
import factor_isai_walk as fw
import mixed_walk as mw
import random_precond_cases as rc
import test_gpu_multigrid as mgmod
from test_gpu_incomplete_factor import Ref as FactorRef, levels

pytestmark = pytest.mark.gpu

KIND_IDS = {"IC": capi.PRECOND_IC, "ILU": capi.PRECOND_ILU, "IRILU": capi.PRECOND_IRILU}
SOLVER_IDS = {"cg": capi.SOLVER_CG, "bicgstab": capi.SOLVER_BICGSTAB, "gmres": capi.SOLVER_GMRES}
LAYOUT_COMPRESSED, LAYOUT_PACKED = 2.0, 3.0  # property spmvLayout


# ---------------------------------------------------------------------------------------------------------------------
# what is compared: the same small surface of a device solver and of a reference standing in for one
# ---------------------------------------------------------------------------------------------------------------------
def counters_of(result, solver):
    """(iterations, norm evaluations, initial and final residual) of an oracle result as the device reports them (the
    criterion counts GKOBiCGStab's half steps, the solver whole ones)."""
    its = result.n_iterations // 2 if solver == "bicgstab" else result.n_iterations
    return (its, result.n_evals, result.initial_residual, result.final_residual)


class OnDevice:
    """A solver that has solved case `key` from zero, and what it left."""

    def __init__(self, s, key, x, perf):
        self.get_property, self.mg_level = s.get_property, s.mg_level
        self.history, self.x = s.history(), x
        self.counters = (perf.n_iterations, perf.n_norm_evals, perf.initial_residual, perf.final_residual)
        self.z = s.apply_preconditioner(rc.case(key).r)


def hierarchy_of(ref):
    """The double-precision reference that owns the hierarchy (the single walk is built on one)."""
    return getattr(ref, "ref", ref)


def facts_of(variant, key, ref):
    """What the generation of `ref` would report: property -> value."""
    family = rc.VARIANTS[variant][0]
    if family in ("factor", "isai"):
        return {"iluLevels": float(len(levels(ref.rp, ref.c, False))), "iluBreakdownRow": -1.0,
                "triangularSolvesInUse": float(family == "isai"),
                "triangularWEntries": float(ref.w_entries) if family == "isai" else 0.0,
                "factorSweepsInUse": float(rc.sweeps_of(variant, key))}
    if family == "cheb":
        return {"chebyshevLambdaMaxInUse": ref.table.lambda_max, "chebyshevLambdaMinInUse": ref.table.lambda_min}
    h = hierarchy_of(ref)
    facts = {"mgLevels": float(h.levels), "mgOperatorComplexity": sum(len(A.cols) for A in h.A) / len(h.A[0].cols),
             "mgCyclePrecisionInUse": float(ref is not h), "coarseVisits": float(getattr(h, "gamma", 1))}
    for l, A in enumerate(h.A):
        facts[f"mgRows{l}"], facts[f"mgNnz{l}"] = float(A.n), float(len(A.cols))
    for l, p in enumerate(getattr(h, "passes", ())):
        facts[f"mgPasses{l}"] = float(p)
    return facts


class FromReference:
    """What a device that follows `ref` to the bit would leave after the same solve: the stand-in of the negative controls."""

    def __init__(self, variant, key, new_id=None):
        ref = rc.reference(variant, key, rc.perm_bytes(new_id) if rc.VARIANTS[variant][0] == "cheb" else None)
        self.facts, self.h = facts_of(variant, key, ref), hierarchy_of(ref)
        self.z = rc.apply_of(variant, key, new_id)(rc.case(key).r)
        out = rc.oracle_solve(variant, key, new_id)
        self.history, self.x, self.counters = out.history, out.x, counters_of(out, rc.params_of(key).solver)

    def get_property(self, name):
        return self.facts[name]

    def mg_level(self, l):
        A = self.h.A[l]
        return A.rp, A.cols, A.vals, (self.h.agg[l] if l + 1 < self.h.levels else None)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison helpers
# ---------------------------------------------------------------------------------------------------------------------
def check_facts(got, want, label):
    for name, value in want.items():
        assert got.get_property(name) == value, f"{label}: {name} is {got.get_property(name)}, the reference's {value}"


def check_apply_and_solve(got, ref, variant, key, new_id, label):
    c = rc.case(key)
    np.testing.assert_array_equal(got.z, rc.apply_of(variant, key, new_id, ref)(c.r), err_msg=f"{label}: z = M^-1 r")
    want = rc.oracle_solve(variant, key, new_id, ref)
    np.testing.assert_array_equal(got.history, want.history, err_msg=f"{label}: residual history")
    np.testing.assert_array_equal(got.x, want.x, err_msg=f"{label}: x")
    assert got.counters == counters_of(want, c.params.solver), f"{label}: {got.counters}"


def check_factor(got, ref, variant, key, new_id=None):
    """IC / ILU / IRILU with the exact solves (IRILU: its sweeps), the factor exact or swept."""
    label = f"{variant}, {rc.describe(key)}"
    check_facts(got, facts_of(variant, key, ref), label)
    check_apply_and_solve(got, ref, variant, key, new_id, label)


def check_isai(got, ref, variant, key, new_id=None):
    """IC / ILU under `triangularSolves isai`."""
    label = f"{variant}, {rc.describe(key)}"
    check_facts(got, facts_of(variant, key, ref), label)
    check_apply_and_solve(got, ref, variant, key, new_id, label)


def check_chebyshev(got, ref, variant, key, new_id=None):
    label = f"{variant} degree {rc.degree_of(key)}, {rc.describe(key)}"
    check_facts(got, facts_of(variant, key, ref), label)
    check_apply_and_solve(got, ref, variant, key, new_id, label)


def check_multigrid(got, ref, variant, key, new_id=None):
    label = f"{variant}, {rc.describe(key)}"
    h = hierarchy_of(ref)
    try:
        mgmod.assert_hierarchy(got, h)
    except AssertionError as e:
        raise AssertionError(f"{label}: {e}") from e
    check_facts(got, facts_of(variant, key, ref), label)
    check_apply_and_solve(got, ref, variant, key, new_id, label)
    if ref is not h:  # (the single walk: subnormal intermediates are not pinned -- there must be none)
        assert ref.smallest_fp32 >= mw.TINY32, f"{label}: {ref.smallest_fp32}"


CHECKS = {"factor": check_factor, "isai": check_isai, "cheb": check_chebyshev, "mg": check_multigrid}


# ---------------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------------
def configure(reg, variant, key):
    """The field of the variant, configured for case `key`; its matrix is not set yet."""
    family, kw = rc.VARIANTS[variant]
    p = rc.params_of(key)
    base = dict(solver=SOLVER_IDS[p.solver], tolerance=rc.TOL, rel_tol=0.0, max_iter=rc.MAX_ITER, krylov_dim=rc.KRYLOV_DIM,
                export_res=1, adapt_min_iter=0, update_init_guess=1,
                renumber=capi.RENUMBER_ON if p.renumber else capi.RENUMBER_OFF)
    if family in ("factor", "isai"):
        base.update(preconditioner=KIND_IDS[kw["kind"]], sparsity_power=kw.get("power", 1))
    elif family == "cheb":
        base.update(preconditioner=capi.PRECOND_CHEBYSHEV)
        if "force_layout" in kw:  # (the half storage would stand in front of the forced layout)
            base.update(symmetric_half=0)
    else:
        base.update(preconditioner=capi.PRECOND_MULTIGRID)
    s = reg.solver(f"rp_{variant}", capi.default_config(**base))
    if family in ("factor", "isai"):
        s.set_triangular_solves("isai" if family == "isai" else "exact")
        s.set_factor_sweeps(rc.sweeps_of(variant, key))
    elif family == "cheb":
        s.set_chebyshev(degree=rc.degree_of(key))
        s.set_property("chebyshevFused", float(kw["fused"]))
        if "force_layout" in kw:
            s.set_property("spmvForceLayout", float(kw["force_layout"]))
        if kw.get("stream"):
            s.set_property("streamAboveBytes", 0.0)
    else:
        mg = dict(mgmod.DEFAULTS, cyclePrecision=kw.get("precision", "double"), aggregation=kw.get("aggregation", "pgm"),
                  aggregatePasses=kw.get("passes", 1), smootherSweeps=kw.get("sweeps", 2), coarseVisits=kw.get("visits", 1))
        s.set_multigrid(**mg)
    return s


def solve(s, key):
    c = rc.case(key)
    s.set_matrix(c.ldu)
    new_id = s.renumbering()
    assert (new_id is not None) == c.params.renumber, rc.describe(key)
    x, perf = s.solve(c.b, np.zeros_like(c.b))
    return new_id, x, perf


def refused_then_exact(s, variant, key):
    """W too wide: the solve is ERR_UNSUPPORTED naming sparsityPower, and the handle solves with the exact solves."""
    label = f"{variant}, {rc.describe(key)}"
    with pytest.raises(capi.OglError) as e:
        solve(s, key)
    assert e.value.status == capi.ERR_UNSUPPORTED and "sparsityPower" in str(e.value), f"{label}: {e.value}"
    s.set_triangular_solves("exact")
    _, x, perf = solve(s, key)
    assert np.isfinite(x).all() and perf.final_residual < perf.initial_residual, label
    assert s.get_property("triangularSolvesInUse") == 0.0, label
    kind, sweeps = rc.VARIANTS[variant][1]["kind"], rc.sweeps_of(variant, key)
    csr = rc.case(key).csr
    exact = fw.Walk(rc._oracle(), *csr, kind, isai=False, sweeps=sweeps) if sweeps else FactorRef(*csr, kind, True)
    r = rc.case(key).r
    np.testing.assert_array_equal(s.apply_preconditioner(r), exact.apply(r), err_msg=label)


def layout_declined(s, variant):
    """Whether the library left the forced layout aside on this pattern (it does not qualify for it)."""
    forced = rc.VARIANTS[variant][1].get("force_layout")
    if forced is None:
        return False
    assert s.get_property("symmetricHalf") == 0.0
    return s.get_property("spmvLayout") != {1: LAYOUT_COMPRESSED, 2: LAYOUT_PACKED}[forced]


def check_chebyshev_path(s, variant, key):
    """Fused only on the whole-matrix half storage, and only when asked."""
    kw = rc.VARIANTS[variant][1]
    half = s.get_property("symmetricHalf") == 1.0 and s.get_property("symmetricHalfPerChunk") == 0.0
    runs_fused = bool(kw["fused"] and half)
    label = f"{variant}, {rc.describe(key)}"
    assert s.get_property("chebyshevFusedInUse") == float(runs_fused), label
    d = rc.degree_of(key)
    assert s.get_property("chebyshevLaunchesPerApply") == (d + 1 if runs_fused else 2 * d + 1), label
    if kw.get("stream"):
        assert s.get_property("spmvStream") == 1.0, label


def run(variant, keys):
    """The variant's field through the cases `keys`; returns (cases run, refused, declined by the forced layout)."""
    family = rc.VARIANTS[variant][0]
    reg = capi.Registry()
    ran, refused, declined = [], [], []
    try:
        for key in keys:
            if not rc.accepts(variant, key):
                continue
            s = configure(reg, variant, key)
            if rc.too_wide(variant, key):
                refused_then_exact(s, variant, key)
                refused.append(key)
                continue
            new_id, x, perf = solve(s, key)
            if layout_declined(s, variant):
                declined.append(key)
                continue
            if family == "cheb":
                check_chebyshev_path(s, variant, key)
            ref = rc.reference(variant, key, rc.perm_bytes(new_id) if family == "cheb" else None)
            CHECKS[family](OnDevice(s, key, x, perf), ref, variant, key, new_id)
            ran.append(key)
    finally:
        reg.close()
    print(variant, "ran", ran, "refused", refused, "declined by the forced layout", declined)
    return ran, refused, declined


@pytest.mark.parametrize("third", [0, 1, 2])
@pytest.mark.parametrize("variant", list(rc.VARIANTS))
def test_drawn_cases(variant, third):
    keys = list(rc.THIRDS[third])
    ran, refused, declined = run(variant, keys)
    wanted = [k for k in keys if rc.accepts(variant, k)]
    assert sorted(ran + refused + declined) == wanted
    assert 2 * len(declined) <= len(wanted), (variant, declined)  # (at most half may be left aside by a forced layout)
    assert ran or not wanted


@pytest.mark.parametrize("variant", list(rc.VARIANTS))
def test_fixed_edges(variant):
    """One row, five rows without a face, a row wider than a wavefront (refused under isai: its row of W_U), a level per row:
    every edge the variant accepts (IC the symmetric forms, IRILU the asymmetric ones)."""
    keys = [k for k in rc.EDGES if rc.accepts(variant, k)]
    assert len(keys) >= 3
    ran, refused, declined = run(variant, keys)
    hubs = [k for k in keys if k in rc.HUBS and rc.VARIANTS[variant][0] == "isai"]
    assert refused == hubs  # (and nothing else is)
    assert sorted(ran + declined) == sorted(k for k in keys if k not in hubs)
