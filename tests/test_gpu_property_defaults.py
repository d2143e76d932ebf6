"""The table of input properties (ogl_amd/csrc/properties.hpp) on the device: a solver that sets every fixed entry to the
table's default is the solver that sets nothing, and every domain of the table still refuses what the hand-written checks
refused -- with OGL_ERR_INVALID at the solve, the keyword and the value in the message."""
import os
import re

import numpy as np
import pytest

from ogl_amd import capi, synthetic

pytestmark = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ogl_amd", "csrc")


@pytest.fixture(scope="module")
def reg():
    r = capi.Registry()
    yield r
    r.close()


def in_use_names():
    """Every report `...InUse` the library writes, by its name in the sources."""
    names = set()
    for name in os.listdir(CSRC):
        with open(os.path.join(CSRC, name)) as f:
            names |= set(re.findall(r'"([A-Za-z_0-9]+InUse)"', f.read()))
    # (not a solver's reports: get_property answers these two from the process-wide allocation ledger, which counts
    #  both solvers of a comparison)
    names -= {"deviceBytesInUse", "pinnedBytesInUse"}
    assert len(names) >= 15
    return sorted(names) + ["spmvLayout"]


def reports(s):
    out = {}
    for key in in_use_names():
        try:
            out[key] = s.get_property(key)
        except capi.OglError:
            out[key] = None  # (never reported by this solve)
    return out


# 84^3 = 1,158 chunks: the smallest box tests/test_gpu_lead_finalizers.py reaches leadFinalizersInUse 1 with, so that the
# leader and held-turn knobs are read
@pytest.mark.parametrize("solver, precond, n, symmetric, kw", [
    (capi.SOLVER_CG, capi.PRECOND_NONE, 8, True, {}),
    (capi.SOLVER_CG, capi.PRECOND_MULTIGRID, 8, True, {}),
    (capi.SOLVER_BICGSTAB, capi.PRECOND_ILU, 8, False, {}),
    (capi.SOLVER_GMRES, capi.PRECOND_ISAI, 8, False, {}),
    (capi.SOLVER_CG, capi.PRECOND_BJ, 84, True, dict(max_block_size=1, max_iter=40)),
])
def test_the_table_default_set_equals_nothing_set(reg, solver, precond, n, symmetric, kw):
    case = synthetic.poisson_case(n, symmetric=symmetric)
    b = synthetic.rhs_for_x_star(case)[0]
    cfg = dict(solver=solver, preconditioner=precond, tolerance=1e-10, rel_tol=0.0, max_iter=200)
    cfg.update(kw)
    got = []
    for explicit in (False, True):
        s = reg.solver(f"defaults_{solver}_{precond}_{n}_{explicit}", capi.default_config(**cfg))
        if explicit:
            for name, default, kind, _ in capi.property_table():
                if kind == "fixed":
                    s.set_property(name, default)
        s.set_matrix(case)
        x, perf = s.solve(b, np.zeros_like(b))
        got.append((x, perf.n_iterations, reports(s)))
    (xa, ia, ra), (xb, ib, rb) = got
    assert ia == ib and ia > 1
    assert ra == rb
    np.testing.assert_array_equal(xa, xb)
    if n == 84:
        assert ra["leadFinalizersInUse"] == 1.0


MG = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_MULTIGRID)
GMRES = dict(solver=capi.SOLVER_GMRES, preconditioner=capi.PRECOND_NONE)
CG = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_NONE)
ILU = dict(solver=capi.SOLVER_BICGSTAB, preconditioner=capi.PRECOND_ILU)
# every entry of the table with a domain: (name, where it is checked, further properties, values just outside and, for a
# whole-numbered domain, one in range that is no whole number).  The bounds: MG_MAX_PASSES 4, MG_MAX_COARSE_VISITS 3,
# MG_MAX_SWEEPS 4, PROJ_MAX 8 (kernels.hpp); an open interval refuses its own ends.
REFUSED = [
    ("aggregation", MG, {}, (-1.0, 2.0, 0.5)),
    ("aggregatePasses", MG, {}, (0.0, 5.0, 1.5)),
    ("aggregateCaching", MG, {}, (-1.0, 1000001.0, 0.5)),
    ("coarseVisits", MG, {}, (0.0, 4.0, 1.5)),
    ("cyclePrecision", MG, {}, (-1.0, 2.0, 0.5)),
    ("smootherSweeps", MG, {}, (0.0, 5.0, 1.5)),
    ("correctionScale", MG, {}, (0.0, 2.0)),
    ("orthoMethod", GMRES, {}, (-1.0, 3.0, 0.5)),
    ("basisPrecision", GMRES, {}, (-1.0, 2.0, 0.5)),
    ("guessProjection", CG, {}, (-1.0, 9.0, 0.5)),
    ("guessProjectionCredit", CG, {}, (-1.0, 2.0, 0.5)),
    ("guessProjectionProducts", CG, {}, (-1.0, 2.0, 0.5)),
    ("triangularSolves", ILU, {}, (-1.0, 2.0, 0.5)),
    ("factorSweeps", ILU, {}, (-1.0, 11.0, 2.5)),
    ("innerRelTol", CG, {"mixedPrecision": 1.0}, (0.0, 1.0)),
]


@pytest.mark.parametrize("name, where, also, bad", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_domain_refuses_what_it_refused(reg, name, where, also, bad):
    case = synthetic.poisson_case(8, symmetric=where is not ILU)
    b = synthetic.rhs_for_x_star(case)[0]
    s = reg.solver(f"refused_{name}", capi.default_config(tolerance=1e-10, rel_tol=0.0, max_iter=200, **where))
    for key, value in also.items():
        s.set_property(key, value)
    s.set_matrix(case)
    default = {n: d for n, d, _, _ in capi.property_table()}[name]
    for value in bad:
        s.set_property(name, value)  # (accepted here: a value is refused at the solve)
        with pytest.raises(capi.OglError) as e:
            s.solve(b, np.zeros_like(b))
        assert e.value.status == capi.ERR_INVALID, e.value
        assert f"{name} {value:g} " in str(e.value), e.value
        s.set_property(name, default)
        _, perf = s.solve(b, np.zeros_like(b))  # the same handle solves
        assert perf.final_residual <= 1e-8
