"""SpMV work mappings and preconditioner-generation variants that only a property selects, against the oracle bit for bit:
the XCD grouping of chunks (xcdGroup: xcd_chunk / xcd_grid pad the grid to a multiple of 8 * group) on the CSR-stream,
compressed and packed-column layouts, the two-round LDS pass of k_spmv_stream (spmvLdsRounds 2), block-Jacobi and ISAI
generation without grouped lanes, ISAI's W kept in its own row order, and the runs of thin levels of IC / ILU / IRILU.
(The half-storage kernels take no group: k_spmv_sym / k_spmv_symx place chunks with the built-in one.)"""
import numpy as np
import pytest

from ogl_amd import capi, synthetic
from helpers import blocked, oracle_csr, oracle_matrix, oracle_matrix_renumbered, oracle_precond_renumbered, to_new
import test_gpu_incomplete_factor as ilu_ref

pytestmark = pytest.mark.gpu

CHUNK = 512
GROUPS = [1, 2, 3, 5, 8, 64, 256]
LAYOUT_CSR, LAYOUT_SELL, LAYOUT_CSR21 = 0.0, 2.0, 3.0
STREAMS = [0.0, 1e18]   # streamAboveBytes: STREAM instantiations forced on / off


def spmv_cfg(compress, **kw):
    base = dict(solver=capi.SOLVER_CG, preconditioner=capi.PRECOND_NONE, tolerance=0.0, rel_tol=0.0, max_iter=10,
                export_res=1, matrix_format=capi.FORMAT_CSR, adapt_min_iter=0, compress_indices=compress)
    base.update(kw)
    return capi.default_config(**base)


def spmv_solver(reg, name, case, compress, stream, props=(), **kw):
    s = reg.solver(name, spmv_cfg(compress, **kw))
    s.set_property("streamAboveBytes", stream)
    s.set_property("spmvBandRows", 0.0)   # (no band-aware order: the XCD grouping places the chunks)
    for k, v in props:
        s.set_property(k, v)
    s.set_matrix(case)
    assert s.get_property("spmvStream") == (1.0 if stream == 0.0 else 0.0)
    return s


def group_sizes(g):
    """Row counts whose chunk count is one below, at and one past 8 * g, with n % 512 = 511, 2 and 1."""
    q = 8 * g
    return [(q - 2) * CHUNK + 511, (q - 1) * CHUNK + 2, q * CHUNK + 1]


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("compress,layout", [(0, LAYOUT_CSR), (1, LAYOUT_SELL)], ids=["csr", "compressed"])
def test_spmv_xcd_group_around_the_grid_padding(oracle, g, compress, layout):
    rng = np.random.default_rng(g)
    reg = capi.Registry()
    try:
        for n in group_sizes(g):
            case = synthetic.poisson_block(n, 1, 1, symmetric=False, off_upper=-0.9, off_lower=-1.1)
            rp, cols, vals = oracle_csr(oracle, case)
            x = rng.uniform(-1, 1, n)
            ref = oracle.spmv(rp, cols, vals, x)
            for stream in STREAMS:
                s = spmv_solver(reg, f"xcd_{n}_{stream}", case, compress, stream, props=[("xcdGroup", float(g))])
                assert s.get_property("spmvLayout") == layout
                for rounds in ((1.0, 2.0) if layout == LAYOUT_CSR else (1.0,)):
                    s.set_property("spmvLdsRounds", rounds)
                    np.testing.assert_array_equal(s.spmv(x), ref, err_msg=f"n={n} stream={stream} rounds={rounds}")
    finally:
        reg.close()


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("solver", [capi.SOLVER_CG, capi.SOLVER_BICGSTAB])
def test_short_solve_on_a_grouped_layout(oracle, g, solver):
    """A few turns with the in-loop SpMV on the CSR-stream layout in the group (two LDS rounds)."""
    n = group_sizes(g)[2]
    sym = solver == capi.SOLVER_CG
    case = synthetic.poisson_block(n, 1, 1, symmetric=sym)
    b = synthetic.rhs_for_x_star(case)[0]
    A, (rp, cols, vals) = oracle_matrix(oracle, case)
    inv = oracle.jacobi_generate_scalar(rp, cols, vals)
    reg = capi.Registry()
    try:
        s = spmv_solver(reg, "xcd_solve", case, 0, 1e18, props=[("xcdGroup", float(g)), ("spmvLdsRounds", 2.0)],
                        solver=solver, preconditioner=capi.PRECOND_BJ, max_iter=9)
        x, perf = s.solve(b, np.zeros_like(b))
        assert s.get_property("spmvLayout") == LAYOUT_CSR
        with blocked(oracle, capi.lib().ogl_reduction_chunk_rows()):
            ref = (oracle.cg if sym else oracle.bicgstab)(A, b, np.zeros_like(b), inv, tolerance=0.0, rel_tol=0.0, max_iter=9)
        assert perf.n_iterations == (ref.n_iterations if sym else ref.n_iterations // 2)
        np.testing.assert_array_equal(s.history(), ref.history)
        np.testing.assert_array_equal(x, ref.x)
    finally:
        reg.close()


def banded_case(n, width, seed):
    """Rows of 2 * width + 1 entries (fewer at the ends): a chunk holds about 512 (2 width + 1) entries."""
    lower = np.repeat(np.arange(n, dtype=np.int32), width)
    upper = lower + np.tile(np.arange(1, width + 1, dtype=np.int32), n)
    keep = upper < n
    lower, upper = lower[keep], upper[keep]
    rng = np.random.default_rng(seed)
    return synthetic.LduCase(n, lower, upper, rng.uniform(40, 50, n), rng.uniform(-1, 1, len(lower)),
                             rng.uniform(-1, 1, len(lower)))


LDS_CASES = {
    "poisson7": lambda: synthetic.poisson_case(21, symmetric=False),          # ~3,580 entries per chunk: two rounds
    "long_rows": lambda: synthetic.long_rows_case(synthetic.poisson_case(22, symmetric=False), 0.3, 22),
    "band5": lambda: banded_case(5 * CHUNK + 3, 5, 1),                        # 11 per row: 5,632 per chunk, two passes
    "band20": lambda: banded_case(4 * CHUNK + 511, 20, 2),                    # 41 per row: 20,992 per chunk, six passes
    "band3_short": lambda: banded_case(CHUNK + 1, 3, 3),                      # 3,584 per chunk, a last chunk of one row
}


@pytest.mark.parametrize("name", sorted(LDS_CASES))
def test_spmv_two_lds_rounds(oracle, name):
    """spmvLdsRounds 2: k_spmv_stream<.., 2>; chunks of more than 2,048 and more than 4,096 entries, rows straddling the
    round boundary (2,048 entries into a pass) and the pass boundary (4,096)."""
    case = LDS_CASES[name]()
    rp, cols, vals = oracle_csr(oracle, case)
    per_chunk = np.diff(rp[::CHUNK])
    assert per_chunk.max() > 2048
    x = np.random.default_rng(7).uniform(-1, 1, case.n_cells)
    ref = oracle.spmv(rp, cols, vals, x)
    reg = capi.Registry()
    try:
        for stream in STREAMS:
            for g in (0.0, 3.0):
                s = spmv_solver(reg, f"lds_{stream}_{g}", case, 0, stream, props=[("spmvLdsRounds", 2.0), ("xcdGroup", g)])
                assert s.get_property("spmvLayout") == LAYOUT_CSR
                np.testing.assert_array_equal(s.spmv(x), ref, err_msg=f"stream={stream} group={g}")
    finally:
        reg.close()


IRREGULAR = {
    # (a hex mesh in a shuffled numbering: after RCM some chunks of the compressed layout need 16-bit deltas, so the
    #  layouts are timed and can be forced; at 41^3 every chunk qualifies with 8-bit ones and the compressed one stays)
    "renumbered_hex": (lambda: synthetic.renumber_case(synthetic.poisson_case(64), 65536), (0, 1, 2)),
    "voronoi": (lambda: synthetic.voronoi_case(70000), (0, 2)),
}


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_spmv_forced_layouts_on_irregular_patterns(oracle, name):
    """spmvForceLayout 0 / 1 / 2 (CSR-stream, compressed, packed columns) on patterns above the tuning size, every XCD
    group, LDS rounds 1 / 2 on the CSR arrays, streamed or not."""
    make, forced = IRREGULAR[name]
    case = make()
    x = np.random.default_rng(5).uniform(-1, 1, case.n_cells)
    reg = capi.Registry()
    try:
        ref = None
        for f in forced:
            for stream in STREAMS:
                s = spmv_solver(reg, f"irr_{f}_{stream}", case, 1, stream, props=[("spmvForceLayout", float(f))])
                assert s.get_property("spmvLayout") == (LAYOUT_CSR, LAYOUT_SELL, LAYOUT_CSR21)[f]
                if ref is None:
                    new_id = s.renumbering()
                    if new_id is None:
                        new_id = np.arange(case.n_cells, dtype=np.int32)
                    _, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
                    ref = oracle.spmv(rp, cols, vals, to_new(x, new_id))[new_id]
                for g in GROUPS:
                    s.set_property("xcdGroup", float(g))
                    for rounds in ((1.0, 2.0) if f == 0 else (1.0,)):
                        s.set_property("spmvLdsRounds", rounds)
                        np.testing.assert_array_equal(s.spmv(x), ref, err_msg=f"layout={f} stream={stream} group={g}")
    finally:
        reg.close()


# ---- preconditioner generation ----
def applied(reg, name, case, props, **kw):
    """z = M^-1 r of the preconditioner a short solve generated with `props` (caller's order)."""
    cfg = capi.default_config(solver=capi.SOLVER_CG if case.symmetric else capi.SOLVER_BICGSTAB, tolerance=0.0,
                              rel_tol=0.0, max_iter=2, export_res=1, adapt_min_iter=0, **kw)
    s = reg.solver(name, cfg)
    for k, v in props:
        s.set_property(k, v)
    s.set_matrix(case)
    s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
    r = np.random.default_rng(11).standard_normal(case.n_cells)
    return s, r, s.apply_preconditioner(r)


def natural_blocks_case():
    """Dense 3 x 3 blocks (every row of a block has the same pattern): natural blocks of 3 under maxBlockSize 4."""
    nb = 200
    lower, upper = [], []
    for b in range(nb):
        r = 3 * b
        lower += [r, r, r + 1]
        upper += [r + 1, r + 2, r + 2]
    rng = np.random.default_rng(4)
    F = len(lower)
    return synthetic.LduCase(3 * nb, np.array(lower, np.int32), np.array(upper, np.int32), rng.uniform(4, 5, 3 * nb),
                             rng.uniform(-1, 1, F), rng.uniform(-1, 1, F))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 7, 8, "natural"])
@pytest.mark.parametrize("lanes", [0.0, 1.0])
def test_block_jacobi_generation_lanes(oracle, k, lanes):
    """bjGroupLanes 0: blocks of 2 .. 8 rows go to the one-thread-per-block kernel (k_bj_generate<LD>)."""
    case = natural_blocks_case() if k == "natural" else synthetic.poisson_case(13, symmetric=False)
    k = 4 if k == "natural" else k
    reg = capi.Registry()
    try:
        s, r, z = applied(reg, "bj", case, [("bjGroupLanes", lanes)], preconditioner=capi.PRECOND_BJ, max_block_size=k,
                          renumber=capi.RENUMBER_OFF)
        assert s.renumbering() is None
    finally:
        reg.close()
    rp, cols, vals = oracle_csr(oracle, case)
    P = oracle.Precond(rp, cols, vals, k)
    assert np.diff(P.block_ptrs).max() == (3 if case.n_cells == 600 else k)
    np.testing.assert_array_equal(z, P.apply(r))


@pytest.mark.parametrize("pc,isai", [(capi.PRECOND_ISAI, "spd"), (capi.PRECOND_GISAI, "general")], ids=["ISAI", "GISAI"])
@pytest.mark.parametrize("lanes", [0.0, 1.0])
def test_isai_generation_lanes(oracle, pc, isai, lanes):
    """isaiGroupLanes 0: rows of W of 4 (ISAI: tril of the 7-point stencil) or 7 entries (GISAI) go to the
    one-thread-per-row kernel (k_isai_generate<8>) instead of k_isai_generate_grp<4 | 8>."""
    case = synthetic.poisson_case(13, symmetric=isai == "spd")
    reg = capi.Registry()
    try:
        s, r, z = applied(reg, "isai", case, [("isaiGroupLanes", lanes)], preconditioner=pc, sparsity_power=1,
                          renumber=capi.RENUMBER_OFF)
        assert s.renumbering() is None
    finally:
        reg.close()
    rp, cols, vals = oracle_csr(oracle, case)
    P = oracle.Precond(rp, cols, vals, isai=isai)
    assert np.diff(P.w_rowptr).max() == (4 if isai == "spd" else 7)
    np.testing.assert_array_equal(z, P.apply(r))


@pytest.mark.parametrize("pc,isai", [(capi.PRECOND_ISAI, "spd"), (capi.PRECOND_GISAI, "general")], ids=["ISAI", "GISAI"])
@pytest.mark.parametrize("sort_rows", [0.0, 1.0])
def test_isai_w_in_its_own_row_order(oracle, pc, isai, sort_rows):
    """isaiSortRows 0: on a shuffled mesh the library renumbers, W (and W^T) go on the compressed layout only where their
    own row order qualifies; the length-sorted copy is never built."""
    case = synthetic.renumber_case(synthetic.poisson_case(40, symmetric=isai == "spd"), 65536)
    reg = capi.Registry()
    try:
        s, r, z = applied(reg, "isai_sort", case, [("isaiSortRows", sort_rows)], preconditioner=pc, sparsity_power=1)
        new_id = s.renumbering()
        assert new_id is not None
        if sort_rows == 0.0:
            assert s.get_property("isaiWSorted") == 0.0 and s.get_property("isaiWtSorted") == 0.0
        else:
            assert s.get_property("isaiWCompressed") == 1.0
    finally:
        reg.close()
    _, (rp, cols, vals) = oracle_matrix_renumbered(oracle, case, new_id)
    P = oracle_precond_renumbered(oracle, case, rp, cols, vals, new_id, isai=isai)
    np.testing.assert_array_equal(z, P.apply(to_new(r, new_id))[new_id])


FACTOR_BOX = 36   # 46,656 rows, 106 levels, the widest of 972 rows


@pytest.fixture(scope="module")
def factor_refs(oracle):
    case_s, case_a = synthetic.poisson_case(FACTOR_BOX), synthetic.poisson_case(FACTOR_BOX, symmetric=False)
    refs = {}
    for kind in ("IC", "ILU", "IRILU"):
        case = case_s if kind == "IC" else case_a
        rp, cols, vals = oracle_csr(oracle, case)
        refs[kind] = (case, ilu_ref.Ref(rp, cols, vals, kind, general=False))
    return refs


@pytest.mark.parametrize("kind", ["IC", "ILU", "IRILU"])
def test_incomplete_factor_thin_level_runs(factor_refs, kind):
    """iluThinRows 1 (every level a launch of its own), 7, 1 << 30 (every level in one single-workgroup run): the factor
    and the solves carry the same bits whichever way the levels are split."""
    case, ref = factor_refs[kind]
    assert max(len(l) for l in ref.fwd) > 256
    r = ilu_ref.rhs(case.n_cells)
    want = ref.apply(r)
    launches = {}
    for thin in (1.0, 7.0, float(1 << 30)):
        reg = capi.Registry()   # (a registry of its own: the factor is generated with this split, not taken from a cache)
        try:
            s = reg.solver(f"thin_{kind}", ilu_ref.cfg(kind, solver=capi.SOLVER_CG if kind == "IC" else capi.SOLVER_BICGSTAB,
                                                       max_iter=2, tolerance=0.0))
            s.set_property("iluThinRows", thin)
            s.set_matrix(case)
            s.solve(np.ones(case.n_cells), np.zeros(case.n_cells))
            np.testing.assert_array_equal(s.apply_preconditioner(r), want, err_msg=f"{kind} iluThinRows {thin}")
            assert s.get_property("iluBreakdownRow") == -1.0
            launches[thin] = s.get_property("iluLaunchesPerApply")
        finally:
            reg.close()
    if kind != "IRILU":
        assert launches[float(1 << 30)] == 2.0
        assert launches[1.0] > launches[7.0] > 2.0
