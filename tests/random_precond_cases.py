"""Drawn irregular systems for the preconditioners that materialise z (IC, ILU, IRILU and their `triangularSolves isai` /
`factorSweeps` forms, Chebyshev, Multigrid): a seeded, stratified list -- the same on a machine without a GPU
(tests/test_random_precond_cases.py: the conditions the list must meet, the references' own soundness, the negative
controls) and on the device (tests/test_gpu_random_preconds.py).  No fixtures, no hypothesis: case(i) can be rebuilt from
its index alone.

case(i) follows the recipe of `systems()` in tests/test_gpu_random_systems.py (faces i -> j with j drawn within `reach`
rows ahead, diagonally dominant, an optional cyclic patch pair); its parameters come from i:

* n: positions 0 and 3 of every four take the next of the fixed sizes 2, 3, 63, 64, 65, C - 1, C, C + 1, 2C - 1, 2C, 2C + 1
  (C: the rows of a reduction chunk), the two others a seeded size from the strata [4, 62], [66, C - 2], [C + 2, 2C - 2],
  [2C + 2, 2C + 80] in turn -- the default distribution of `systems()` gives one system above one chunk in 60;
* symmetric: cases 0, 1 of every four (in pairs, so that the numbering below is not tied to the symmetry);
* a cyclic pair: the first four of every eight;
* reach in {3, 40, 1000} and per_row in 1 .. 5 along Latin squares of i, so that neither is tied to i % 3 (the sweeps a
  case is factorised with) or i % 5 (the degree it is given);
* renumber (the device copy in a numbering of its own): odd i;
* GMRES(5) instead of CG / BiCGStab: every third case, along a third Latin square, where the system has more rows than
  the restart length.

The references (test_gpu_incomplete_factor.Ref, factor_isai_walk.Walk, chebyshev_walk.Walk, test_gpu_multigrid.Ref, the
pass / visit references and mg_single_walk.SingleWalk) are imported unchanged; `reference(variant, key)` builds each once
per process -- do not change what it returns."""
import functools
from collections import namedtuple

import numpy as np

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, to_new
import chebyshev_walk as cw
import factor_isai_walk as fw
import mg_single_walk as sw
from test_gpu_incomplete_factor import Ref as FactorRef
from test_gpu_multigrid import DEFAULTS as MG_DEFAULTS, Ref as MgRef
from test_gpu_multigrid_aggregation import PassRef
from test_gpu_multigrid_visits import VisitRef

N_CASES = 48
THIRDS = (range(0, 16), range(16, 32), range(32, 48))
REACHES = (3, 40, 1000)
SWEEPS = (0, 1, 3)           # factorSweeps of the isai variants, by i % 3
DEGREES = (1, 2, 3, 4, 16)   # chebyshevDegree, by i % 5
TOL, MAX_ITER, KRYLOV_DIM = 1e-12, 12, 5
HUB_WIDTH = 70

Params = namedtuple("Params", "key n reach per_row symmetric cyclic renumber solver seed")


def chunk_rows():
    return capi.lib().ogl_reduction_chunk_rows()


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def fixed_sizes():
    C = chunk_rows()
    return (2, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1)


def strata():
    C = chunk_rows()
    return ((4, 62), (66, C - 2), (C + 2, 2 * C - 2), (2 * C + 2, 2 * C + 80))


@functools.lru_cache(maxsize=None)
def params(i):
    """The parameters of drawn case i (0 <= i < N_CASES)."""
    assert 0 <= i < N_CASES
    if i % 4 in (0, 3):
        slot = 2 * (i // 4) + (i % 4 == 3)
        n = fixed_sizes()[slot % len(fixed_sizes())]
    else:
        slot = 2 * (i // 4) + (i % 4 == 2)
        lo, hi = strata()[slot % 4]
        n = int(np.random.default_rng([7, i]).integers(lo, hi + 1))
    symmetric = i % 4 < 2
    q = i // 3
    # (not below krylovDim + 1 rows: there one cycle exhausts the Krylov space and the loop divides 0 by 0, whatever the
    #  preconditioner)
    gmres = (i + 2 * q) % 3 == 0 and n > KRYLOV_DIM
    return Params(key=i, n=n, reach=REACHES[(i + q) % 3], per_row=1 + (i + i // 5) % 5, symmetric=symmetric,
                  cyclic=i % 8 < 4, renumber=i % 2 == 1, solver="gmres" if gmres else "cg" if symmetric else "bicgstab",
                  seed=1000 + i)


def narrow(i):
    """The cases sparsityPower 2 is used with: at reach 3 with at most 3 faces per row W stays within the device's rows."""
    p = params(i)
    return p.reach == 3 and p.per_row <= 3


def _ldu(n, pairs, symmetric, rng, ifaces=()):
    """The diagonally dominant lduMatrix of `systems()` on the faces `pairs` (owner < neighbour, sorted)."""
    pairs = np.array(sorted(pairs), dtype=np.int32).reshape(-1, 2)
    f = len(pairs)
    upper = rng.uniform(-1, 0, f)
    lower = None if symmetric else rng.uniform(-1, 0, f)
    ifaces = list(ifaces(rng)) if callable(ifaces) else list(ifaces)
    diag = np.full(n, 1.0)
    np.add.at(diag, pairs[:, 0], np.abs(upper))
    np.add.at(diag, pairs[:, 1], np.abs(upper if symmetric else lower))
    for itf in ifaces:
        np.add.at(diag, itf.face_cells, np.abs(itf.bou_coeffs))
    return synthetic.LduCase(n, pairs[:, 0].copy(), pairs[:, 1].copy(), diag, upper, lower, ifaces)


def _drawn(p):
    rng = np.random.default_rng(p.seed)
    n = p.n
    pairs = set()
    for i in range(n - 1):
        for j in rng.integers(i + 1, min(n, i + 1 + p.reach), p.per_row):
            pairs.add((i, int(j)))

    def cyclic(rng):
        if not p.cyclic:
            return []
        m = int(rng.integers(1, min(8, n) + 1))
        a = rng.choice(n, m, replace=False).astype(np.int32)
        b = rng.choice(n, m, replace=False).astype(np.int32)
        c = rng.uniform(0, 0.5, m)
        return [synthetic.Interface(synthetic.IFACE_CYCLIC, a, c, -1, 1),
                synthetic.Interface(synthetic.IFACE_CYCLIC, b, c if p.symmetric else rng.uniform(0, 0.5, m), -1, 0)]
    return _ldu(n, pairs, p.symmetric, rng, cyclic)


def _edge(name, n, symmetric, solver=None):
    return Params(key=name, n=n, reach=0, per_row=0, symmetric=symmetric, cyclic=False, renumber=False,
                  solver=solver or ("cg" if symmetric else "bicgstab"), seed=0)


def _hub_pairs(n):
    """Row 3 coupled to HUB_WIDTH later rows (every second one), over a sparse chain: its row of the matrix is wider than a
    wavefront, its row of W_U too, while every row of W_L stays narrow."""
    pairs = {(i, i + 1) for i in range(0, n - 1, 3)}
    pairs |= {(3, 5 + 2 * k) for k in range(HUB_WIDTH)}
    return pairs


# the fixed edges: name -> (parameters, faces)
def _edges():
    C = chunk_rows()
    hub_n = 5 + 2 * HUB_WIDTH + 4
    return {
        "one_row": (_edge("one_row", 1, True), set()),
        "diagonal5_sym": (_edge("diagonal5_sym", 5, True), set()),
        "diagonal5_asym": (_edge("diagonal5_asym", 5, False), set()),
        "hub_sym": (_edge("hub_sym", hub_n, True), _hub_pairs(hub_n)),
        "hub_asym": (_edge("hub_asym", hub_n, False, "gmres"), _hub_pairs(hub_n)),
        "chain_sym": (_edge("chain_sym", C + 1, True), {(i, i + 1) for i in range(C)}),  # a level per row
        "chain_asym": (_edge("chain_asym", C + 1, False), {(i, i + 1) for i in range(C)}),
    }


EDGES = ("one_row", "diagonal5_sym", "diagonal5_asym", "hub_sym", "hub_asym", "chain_sym", "chain_asym")
HUBS = ("hub_sym", "hub_asym")


def params_of(key):
    return params(key) if isinstance(key, int) else _edges()[key][0]


Case = namedtuple("Case", "params ldu b r csr")


@functools.lru_cache(maxsize=None)
def case(key):
    """Case `key` (an index below N_CASES or the name of a fixed edge): (params, the lduMatrix, b, r, (rowptr, cols, vals)
    as the reference assembles it); b and r from default_rng(i) (the edges: from their position behind the drawn ones).
    Built once; do not change it."""
    p = params_of(key)
    if isinstance(key, int):
        ldu, seed = _drawn(p), key
    else:
        ldu, seed = _ldu(p.n, _edges()[key][1], p.symmetric, np.random.default_rng(5000 + EDGES.index(key))), \
            N_CASES + EDGES.index(key)
    rng = np.random.default_rng(seed)
    b, r = rng.uniform(-1, 1, p.n), rng.standard_normal(p.n)
    return Case(p, ldu, b, r, oracle_csr(_oracle(), ldu))


def describe(key):
    p = params_of(key)
    return (f"case {key!r}: n {p.n} reach {p.reach} per_row {p.per_row} {'symmetric' if p.symmetric else 'asymmetric'}"
            f"{' cyclic' if p.cyclic else ''}{' renumbered' if p.renumber else ''} {p.solver}")


def host_numbering(key):
    """new_id the library gives the device copy of a case with `renumber on` (computed on the host), None with `off`."""
    if not params_of(key).renumber:
        return None
    renumbered, new_id = capi.host_pattern_renumbered(case(key).ldu)[4]
    return new_id if renumbered else None


# ---------------------------------------------------------------------------------------------------------------------
# variants: what a solver is configured with, and the reference of it
# ---------------------------------------------------------------------------------------------------------------------
# name -> (family, keywords); the keyword values that depend on the case come from the functions below
VARIANTS = {
    "IC": ("factor", dict(kind="IC")),
    "ILU": ("factor", dict(kind="ILU")),
    "IRILU": ("factor", dict(kind="IRILU")),
    "IC_swept": ("factor", dict(kind="IC", swept=True)),
    "ILU_swept": ("factor", dict(kind="ILU", swept=True)),
    "IRILU_swept": ("factor", dict(kind="IRILU", swept=True)),
    "IC_isai_p1": ("isai", dict(kind="IC", power=1)),
    "ILU_isai_p1": ("isai", dict(kind="ILU", power=1)),
    "IC_isai_p2": ("isai", dict(kind="IC", power=2)),
    "ILU_isai_p2": ("isai", dict(kind="ILU", power=2)),
    "cheb_fused": ("cheb", dict(fused=1)),
    "cheb_unfused": ("cheb", dict(fused=0)),
    "cheb_compressed": ("cheb", dict(fused=0, force_layout=1)),
    "cheb_packed": ("cheb", dict(fused=0, force_layout=2)),
    "cheb_stream": ("cheb", dict(fused=0, stream=True)),
    "mg_double": ("mg", dict(precision="double")),
    "mg_single": ("mg", dict(precision="single")),
    "mg_hashed2": ("mg", dict(aggregation="hashed", passes=2)),
    "mg_visits2": ("mg", dict(sweeps=2, visits=2)),
}


def position(key):
    return key if isinstance(key, int) else N_CASES + EDGES.index(key)


def sweeps_of(variant, key):
    """factorSweeps of a factor variant on a case."""
    family, kw = VARIANTS[variant]
    if family == "isai":
        return SWEEPS[position(key) % 3]
    return (3 if position(key) % 2 else 1) if kw.get("swept") else 0


def degree_of(key):
    """chebyshevDegree of a case: by i % 5 on the drawn ones, the default on the edges."""
    return DEGREES[key % 5] if isinstance(key, int) else cw.DEFAULT_DEGREE


def accepts(variant, key):
    """Whether the variant is run on the case at all: IC on symmetric matrices, IRILU on asymmetric ones, sparsityPower 2
    on the narrow cases and the small edges."""
    family, kw = VARIANTS[variant]
    symmetric = params(key).symmetric if isinstance(key, int) else not key.endswith("_asym")
    if family in ("factor", "isai"):
        if kw["kind"] == "IC" and not symmetric:
            return False
        if kw["kind"] == "IRILU" and symmetric:
            return False
        if kw.get("power") == 2 and isinstance(key, int) and not narrow(key):
            return False
    return True


@functools.lru_cache(maxsize=None)
def reference(variant, key, new_id=None):
    """The reference of a variant on a case, built once.  Factors and hierarchies belong to the caller's numbering whatever
    the device copy's; Chebyshev's walk is that of the system permuted by new_id (bytes of the int32 array, or None)."""
    family, kw = VARIANTS[variant]
    oracle = _oracle()
    rp, cols, vals = case(key).csr
    if family == "factor":
        if not kw.get("swept"):
            return FactorRef(rp, cols, vals, kw["kind"], True)
        return fw.Walk(oracle, rp, cols, vals, kw["kind"], isai=False, sweeps=sweeps_of(variant, key))
    if family == "isai":
        return fw.Walk(oracle, rp, cols, vals, kw["kind"], isai=True, power=kw["power"], sweeps=sweeps_of(variant, key))
    if family == "cheb":
        if new_id is not None:
            rp, cols, vals, _ = oracle.permute_csr(rp, cols, vals, np.frombuffer(new_id, np.int32))
        return cw.Walk(oracle, rp, cols, vals, degree=degree_of(key))
    if "aggregation" in kw:
        return PassRef(oracle, rp, cols, vals, **dict(MG_DEFAULTS, aggregation=kw["aggregation"], aggregatePasses=kw["passes"]))
    if "visits" in kw:
        return VisitRef(oracle, rp, cols, vals, **MG_DEFAULTS).with_gamma(kw["visits"])
    if kw["precision"] == "single":  # (on the double reference's own hierarchy)
        return sw.SingleWalk(reference("mg_double", key))
    return MgRef(oracle, rp, cols, vals, **MG_DEFAULTS)


def w_width(walk):
    """The widest row of W_L and of W_U of an isai walk."""
    return max(max(len(r) for r in walk.rows), max(len(r) for r in walk.rows_t))


def too_wide(variant, key):
    """Whether the variant must be refused on the case: a row of W_L or of W_U wider than the device's rows."""
    return VARIANTS[variant][0] == "isai" and w_width(reference(variant, key)) > fw.MAX_W_ROW


def perm_bytes(new_id):
    return None if new_id is None else np.ascontiguousarray(new_id, np.int32).tobytes()


def apply_of(variant, key, new_id=None, ref=None):
    """r -> z in the caller's order, with the reference of the variant (or `ref`, a deliberately wrong one)."""
    family = VARIANTS[variant][0]
    if family != "cheb":
        ref = ref or reference(variant, key)
        return ref.apply
    ref = ref or reference(variant, key, perm_bytes(new_id))
    if new_id is None:
        return ref.apply
    return lambda r: ref.apply(to_new(r, new_id))[new_id]


def oracle_solve(variant, key, new_id=None, ref=None):
    """The oracle's solve of case `key` from zero (tolerance 1e-12, relTol 0, maxIter 12; CG | BiCGStab | GMRES(5) as the case
    says) in the device's reduction tree, on the system permuted by new_id, with the variant's reference (or `ref`) called
    back as the preconditioner; x comes back in the caller's order."""
    oracle = _oracle()
    c = case(key)
    rp, cols, vals = c.csr
    b = c.b
    apply = apply_of(variant, key, new_id, ref)
    if new_id is not None:
        new_id = np.asarray(new_id)
        rp, cols, vals, _ = oracle.permute_csr(rp, cols, vals, new_id)
        b = to_new(b, new_id)
        P = oracle.CallbackPrecond(lambda r: to_new(apply(r[new_id]), new_id))
    else:
        P = oracle.CallbackPrecond(apply)
    A = oracle.DistMatrix(rp, cols, vals)
    kw = dict(tolerance=TOL, rel_tol=0.0, max_iter=MAX_ITER)
    with blocked(oracle, chunk_rows()):
        if c.params.solver == "gmres":
            out = oracle.gmres(A, b, np.zeros_like(b), P, krylov_dim=KRYLOV_DIM, **kw)
        else:
            out = getattr(oracle, c.params.solver)(A, b, np.zeros_like(b), P, **kw)
    if new_id is not None:
        out.x = out.x[new_id]
    return out
