"""The oracle's callback preconditioner (ORC_PRECOND_CALLBACK) and the references built on it, on the CPU alone.

1. helpers.blocked nests: a reference that enters a block of its own while it is called back from a solve under an outer
   one leaves the outer block's reduction tree in place.
2. A callback that wraps Precond.apply of a kind the C loops apply themselves gives the same solve, bit for bit, as the kind
   passed directly -- the callback path adds nothing of its own.
3. The conditions that the GPU comparisons (test_gpu_precond_solves.py) rely on, asserted on the references alone: every
   solve that runs until the criterion stops it does so by the tolerance, after at least 10 checks, at the solution, and
   every Multigrid hierarchy has at least 3 levels."""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_precond_renumbered, to_new
import precond_cases as pc


def test_blocked_nests(oracle):
    v = np.random.default_rng(1).standard_normal(1500)
    sequential = oracle.dot(v, v)
    with blocked(oracle, 512):
        want = oracle.dot(v, v)
    assert want != sequential  # (the two trees do differ on this vector: the test can tell them apart)
    assert oracle.dot(v, v) == sequential
    with blocked(oracle, 512):
        with blocked(oracle, 512):
            assert oracle.dot(v, v) == want
        assert oracle.dot(v, v) == want  # between the inner exit and the outer exit
        with blocked(oracle, 64):       # an inner block of another chunk size hands the outer one's back
            assert oracle.dot(v, v) != want
        assert oracle.dot(v, v) == want
    assert oracle.dot(v, v) == sequential


DIRECT_KINDS = {
    "BJ1": dict(max_block_size=1),
    "BJ4": dict(max_block_size=4),
    "ISAI": dict(isai="spd"),
    "GISAI": dict(isai="general"),
}


def same_solve(a, b):
    np.testing.assert_array_equal(a.history, b.history)
    np.testing.assert_array_equal(a.x, b.x)
    assert a.n_iterations == b.n_iterations and a.n_evals == b.n_evals
    assert a.final_residual == b.final_residual and a.initial_residual == b.initial_residual


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres"])
@pytest.mark.parametrize("kind", sorted(DIRECT_KINDS))
@pytest.mark.parametrize("name", ["sym", "asym"])
def test_callback_equals_the_kind_passed_directly(oracle, name, kind, solver):
    case, b, xs, (rp, cols, vals) = pc.system(name)
    A = oracle.DistMatrix(rp, cols, vals)
    P = oracle.Precond(rp, cols, vals, **DIRECT_KINDS[kind])
    calls = []

    def apply(r):
        calls.append(1)
        return P.apply(r)
    direct = pc.oracle_solve(A, b, P, solver)
    through = pc.oracle_solve(A, b, pc.callback(apply), solver)
    assert len(calls) >= direct.n_iterations - 1 > 0  # (the callback really was the preconditioner)
    assert np.isfinite(direct.history).all()
    same_solve(through, direct)


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres"])
@pytest.mark.parametrize("kind", ["BJ4", "ISAI"])
def test_callback_equals_the_kind_passed_directly_renumbered(oracle, kind, solver):
    """The renumbered system with the preconditioner of the caller's numbering (helpers.oracle_precond_renumbered), and
    the callback that carries r back to the caller's order and z forward around the caller's own Precond: for BJ(4) the
    same blocks applied through new_id.  (ISAI: the callback wraps the renumbered object itself.)"""
    case = pc.system("shuffled14")[0]
    renumbered, new_id = capi.host_pattern_renumbered(case)[4]
    assert renumbered
    b = to_new(pc.system("shuffled14")[1], new_id)
    rp0, cols0, vals0 = oracle_csr(oracle, case)
    rp, cols, vals, _ = oracle.permute_csr(rp0, cols0, vals0, new_id)
    A = oracle.DistMatrix(rp, cols, vals)
    P = oracle_precond_renumbered(oracle, case, rp, cols, vals, new_id, **DIRECT_KINDS[kind])
    if kind == "BJ4":
        P0 = oracle.Precond(rp0, cols0, vals0, 4)
        through = pc.callback(P0.apply, new_id)
    else:
        through = pc.callback(P.apply)
    same_solve(pc.oracle_solve(A, b, through, solver), pc.oracle_solve(A, b, P, solver))


def host_numbering(name):
    renumbered, new_id = capi.host_pattern_renumbered(pc.system(name)[0])[4]
    assert renumbered
    return new_id


@pytest.mark.parametrize("name,kind,solver", pc.MATRIX + pc.OTHER, ids=lambda v: str(v))
def test_the_references_pin_what_they_are_meant_to(name, kind, solver):
    new_id = host_numbering(name) if name == "shuffled14" else None
    ref = pc.reference(name, kind, solver, new_id=new_id)
    pc.check_sound(ref, pc.system(name)[2], bicgstab=solver == "bicgstab")
    if kind == "MG":
        assert pc.precond_ref(name, kind).levels >= 3


@pytest.mark.parametrize("name", ["chunks48", "chunks48_asym"])
def test_the_leader_turn_systems_have_48_chunks(name):
    case = pc.system(name)[0]
    assert -(-case.n_cells // pc.chunk_rows()) == 48 and case.symmetric == (name == "chunks48")
