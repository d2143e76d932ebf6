"""Reference solves with the preconditioners that materialise z and that the oracle's C loops cannot apply themselves (IC,
ILU, IRILU, Multigrid): the oracle's Krylov loop in the device's reduction tree, with the NumPy reference of the kind's
apply (`Ref` of tests/test_gpu_incomplete_factor.py and of tests/test_gpu_multigrid.py, unchanged) called back as its
preconditioner (oracle.CallbackPrecond).  Shared by the CPU test of the references (test_oracle_precond_callback.py), the
single-rank GPU comparison (test_gpu_precond_solves.py) and the multi-rank worker (precond_ranks_worker.py): every
reference is computed once per process and left unchanged."""
import functools

import numpy as np

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, to_new
from test_gpu_incomplete_factor import Ref as FactorRef
from test_gpu_multigrid import DEFAULTS as MG_DEFAULTS, Ref as MgRef

TOL, MAX_ITER, KRYLOV_DIM = 1e-9, 300, 20
FACTOR_KINDS = ("IC", "ILU", "IRILU")
KIND_IDS = {"IC": capi.PRECOND_IC, "ILU": capi.PRECOND_ILU, "IRILU": capi.PRECOND_IRILU, "MG": capi.PRECOND_MULTIGRID}
SOLVER_IDS = {"cg": capi.SOLVER_CG, "bicgstab": capi.SOLVER_BICGSTAB, "gmres": capi.SOLVER_GMRES}

SYSTEMS = {
    "sym": lambda: synthetic.poisson_case(12),                                   # 1,728 rows: 4 chunks
    "asym": lambda: synthetic.poisson_case(12, symmetric=False),
    "shuffled14": lambda: synthetic.renumber_case(synthetic.poisson_case(14), 4096),  # (what `renumber` on reorders)
    "voronoi": lambda: synthetic.voronoi_case(3000),
    "chunks48": lambda: synthetic.poisson_block(32, 32, 24),                     # 24,576 rows: the leader turn's smallest
    "chunks48_asym": lambda: synthetic.poisson_block(32, 32, 24, symmetric=False, off_upper=-0.9, off_lower=-1.1),
}

# kinds x solvers on the two 12^3 systems
MATRIX = [("sym", kind, solver) for kind in ("IC", "MG") for solver in ("cg", "bicgstab", "gmres")] + \
         [("asym", kind, solver) for kind in ("ILU", "IRILU", "MG") for solver in ("bicgstab", "gmres")]
# the other systems whose solves run until the criterion stops them
OTHER = [("shuffled14", "IC", "cg"), ("shuffled14", "MG", "cg"), ("voronoi", "IC", "cg"), ("voronoi", "MG", "cg")]


def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def system(name):
    """(case, b, x*, (rowptr, cols, vals)) of a named system."""
    case = SYSTEMS[name]()
    b, xs = synthetic.rhs_for_x_star(case)
    return case, b, xs, oracle_csr(_oracle(), case)


def make_ref(kind, rowptr, cols, vals):
    """The reference of a kind's apply on the matrix (rowptr, cols, vals), in that matrix's numbering."""
    if kind == "MG":
        return MgRef(_oracle(), rowptr, cols, vals, **MG_DEFAULTS)
    return FactorRef(rowptr, cols, vals, kind, True)


@functools.lru_cache(maxsize=None)
def precond_ref(name, kind):
    return make_ref(kind, *system(name)[3])


def callback(apply, new_id=None):
    """The oracle's preconditioner that calls `apply` (r -> z in the caller's numbering).  new_id: the oracle solves the
    system renumbered by it (new_id[caller row] = row there) -- r is carried back to the caller's order, z forward; the
    factor and the hierarchy belong to the caller's numbering."""
    if new_id is None:
        return _oracle().CallbackPrecond(apply)
    new_id = np.asarray(new_id)
    return _oracle().CallbackPrecond(lambda r: to_new(apply(r[new_id]), new_id))


def oracle_solve(A, b, P, solver, tolerance=TOL, max_iter=MAX_ITER, krylov_dim=KRYLOV_DIM):
    """The oracle's solve in the device's reduction tree."""
    oracle = _oracle()
    kw = dict(tolerance=tolerance, rel_tol=0.0, max_iter=max_iter)
    with blocked(oracle, chunk_rows()):
        if solver == "gmres":
            return oracle.gmres(A, b, np.zeros_like(b), P, krylov_dim=krylov_dim, **kw)
        return getattr(oracle, solver)(A, b, np.zeros_like(b), P, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, kind, solver, perm, crit, apply):
    oracle = _oracle()
    case, b, xs, (rp, cols, vals) = system(name)
    apply = apply or precond_ref(name, kind).apply
    new_id = None if perm is None else np.frombuffer(perm, np.int32)
    if new_id is not None:
        rp, cols, vals, _ = oracle.permute_csr(rp, cols, vals, new_id)
        b = to_new(b, new_id)
    ref = oracle_solve(oracle.DistMatrix(rp, cols, vals), b, callback(apply, new_id), solver, **dict(crit))
    if new_id is not None:
        ref.x = ref.x[new_id]  # back to the caller's order
    return ref


def reference(name, kind, solver, new_id=None, apply=None, **crit):
    """The oracle's Result for a named system (permuted by new_id, x back in the caller's order).  apply: another r -> z
    than the kind's reference (a deliberately wrong one, for the negative controls).  Computed once; do not change it."""
    perm = None if new_id is None else np.ascontiguousarray(new_id, np.int32).tobytes()
    return _reference(name, kind, solver, perm, tuple(sorted(crit.items())), apply)


def check_sound(ref, xs, max_iter=MAX_ITER, bicgstab=False):
    """What a case that runs until the criterion stops it must satisfy to pin anything: it stops by the tolerance before
    max_iter, after at least 10 checks, at the solution."""
    cap = 2 * max_iter if bicgstab else max_iter  # (the criterion counts GKOBiCGStab's half steps)
    assert ref.final_residual <= TOL and ref.n_iterations <= cap, (ref.n_iterations, ref.final_residual)
    assert ref.n_iterations >= 10, ref.n_iterations
    assert np.abs(ref.x - xs).max() <= 1e-6, np.abs(ref.x - xs).max()
