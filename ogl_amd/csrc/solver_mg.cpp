// solver_mg.cpp -- preconditioner Multigrid (Preconditioner.H:259-341): generation of the aggregation hierarchy on the
// device, one V-cycle as the apply (coarseVisits > 1: every coarse level but the coarsest visited that often per visit of
// its parent; cyclePrecision single: on binary32 operands; smootherSweeps sweeps before and after the coarse correction,
// which is scaled by correctionScale), and the entry points that hand the hierarchy out.  Kernels: kernels_mg.hip; the
// contract: DESIGN.md section 7b.
#include "solver_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace ogl;

namespace {

// buffers of the hierarchy only grow: a time-step loop whose sizes repeat stops allocating
template <class T>
int grow(DevBuf<T> &b, size_t count, hipStream_t st)
{
    if (b.p && b.cap >= count) return OGL_OK;
    return b.alloc(std::max<size_t>(1, count + count / 8), st);
}

int read_i32(const int32_t *dev, int32_t *host, hipStream_t st)
{
    OGL_HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    return OGL_OK;
}

}  // namespace

int ogl_solver::check_multigrid_keywords()
{
    // (the keywords of the preconditioner's sub-dictionary travel as properties, Preconditioner.H:297-317)
    if (prop("cycle", 0.0) != 0.0)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner Multigrid: cycle %s is not built (only cycle v)",
                    prop("cycle", 0.0) == 1.0 ? "w" : "f");
    if (prop("zeroGuess", 1.0) == 0.0)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner Multigrid: zeroGuess false is not built");
    if (prop("maxLevels", 9.0) < 0.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: maxLevels %d is negative", (int)prop("maxLevels", 9.0));
    if (prop("coarseSolverIters", 4.0) < 0.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: coarseSolverIters %d is negative",
                    (int)prop("coarseSolverIters", 4.0));
    const double aggregation = prop("aggregation", 0.0), passes = prop("aggregatePasses", 1.0);
    if (aggregation != 0.0 && aggregation != 1.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: aggregation %g is neither 0 (pgm) nor 1 (hashed)", aggregation);
    if (!(passes >= 1.0 && passes <= (double)MG_MAX_PASSES) || passes != (double)(int)passes)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: aggregatePasses %g outside [1, %d]", passes, MG_MAX_PASSES);
    const double visits = prop("coarseVisits", 1.0);
    if (!(visits >= 1.0 && visits <= (double)MG_MAX_COARSE_VISITS) || visits != (double)(int)visits)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: coarseVisits %g outside [1, %d]", visits, MG_MAX_COARSE_VISITS);
    const double precision = prop("cyclePrecision", 0.0);
    if (precision != 0.0 && precision != 1.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: cyclePrecision %g is neither 0 (double) nor 1 (single)",
                    precision);
    const double sweeps = prop("smootherSweeps", 2.0);
    if (!(sweeps >= 1.0 && sweeps <= (double)MG_MAX_SWEEPS) || sweeps != (double)(int)sweeps)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: smootherSweeps %g outside [1, %d]", sweeps, MG_MAX_SWEEPS);
    // (a condition, not a tuning value: with an exact coarse solve the correction step I - scale Pi stops contracting at 2)
    const double scale = prop("correctionScale", 1.0);
    if (!(scale > 0.0 && scale < 2.0))
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: correctionScale %g outside (0, 2)", scale);
    return OGL_OK;
}

// This solver's side of an apply of the hierarchy (its own or a stored one): coarseVisits, and how often one apply then
// visits every level -- level 0 once, every level below it coarseVisits times per visit of its parent, the coarsest as
// often as its parent.  A hierarchy too deep for that many visits is refused here, before any apply.
int ogl_solver::prepare_multigrid_apply()
{
    const MultigridPart &M = precond_data->mg;
    mg_coarse_visits = (int)prop("coarseVisits", 1.0);
    props["coarseVisits"] = (double)mg_coarse_visits;
    // smootherSweeps and correctionScale are the applier's too; check_multigrid_keywords has refused the rest, and an
    // apply never runs with a count the ping-pong of the sweeps was not built for
    mg_sweeps = (int)prop("smootherSweeps", 2.0);
    mg_scale = prop("correctionScale", 1.0);
    if (mg_sweeps < 1 || mg_sweeps > MG_MAX_SWEEPS || !(mg_scale > 0.0 && mg_scale < 2.0))
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: smootherSweeps %d outside [1, %d] or correctionScale %g outside (0, 2)",
                    mg_sweeps, MG_MAX_SWEEPS, mg_scale);
    props["smootherSweeps"] = (double)mg_sweeps;
    props["correctionScale"] = mg_scale;
    std::vector<double> visits((size_t)M.n_levels, 1.0);
    double total = 0.0;
    for (int l = 0; l < M.n_levels; ++l) {
        if (l > 0) visits[(size_t)l] = visits[(size_t)l - 1] * (l + 1 < M.n_levels ? (double)mg_coarse_visits : 1.0);
        total += visits[(size_t)l];
    }
    if (total > (double)MG_MAX_VISITS_PER_APPLY)
        return fail(OGL_ERR_UNSUPPORTED,
                    "preconditioner Multigrid: coarseVisits %d on %d levels makes %.0f level visits per apply (at most %d): "
                    "raise aggregatePasses for a shallower hierarchy, or lower coarseVisits or maxLevels",
                    mg_coarse_visits, M.n_levels, total, MG_MAX_VISITS_PER_APPLY);
    for (int l = 0; l < M.n_levels; ++l) props["mgVisits" + std::to_string(l)] = visits[(size_t)l];
    // cyclePrecision is the applier's too: a stored hierarchy gets its binary32 twin when a solver first asks for it
    mg_single = prop("cyclePrecision", 0.0) == 1.0;
    if (mg_single) OGL_TRY(prepare_multigrid_single());
    props["mgCyclePrecisionInUse"] = mg_single ? 1.0 : 0.0;
    return OGL_OK;
}

// cyclePrecision single ("the cycle in single precision"): what an apply on binary32 operands needs
// besides the hierarchy.  (1) The levels' twin -- values and 1 / d rounded from the stored doubles by one kernel per level,
// and the levels' vectors -- once per generated hierarchy, whoever applies it.  (2) Where level 0 is the system matrix in
// the in-loop layout, the fp32 copy the mixed-precision mode uses (Fp32Dev), refreshed per values epoch.  A value that is
// finite in fp64 and not in binary32 fails the solve; what failed is left stale, so that the next solve converts -- and
// reports -- again.
int ogl_solver::prepare_multigrid_single()
{
    hipStream_t st = reg->stream;
    const MultigridPart &M = precond_data->mg;
    const int nl = M.n_levels;
    OGL_TRY(grow(M.bad, (size_t)nl + 1, st));
    bool converted = false;
    if (M.twin_of != M.generated) {
        OGL_HIP_CHECK(hipMemsetAsync(M.bad.p, 0x7f, ((size_t)nl + 1) * sizeof(int32_t), st));
        for (int l = 0; l < nl; ++l) {
            MgLevel &L = *M.levels[(size_t)l];
            const size_t nv = (size_t)L.n + 4;  // (a trailing pair access of the last odd row stays inside)
            OGL_TRY(grow(L.inv_d32, nv, st));
            if (L.own) OGL_TRY(grow(L.vals32, (size_t)L.nnz + 2, st));
            for (DevBuf<float> *v : {&L.b32, &L.xa32, &L.xb32, &L.t32}) OGL_TRY(grow(*v, nv, st));
            if (l == nl - 1) {
                OGL_TRY(grow(L.r32, nv, st));
                OGL_TRY(grow(L.p32, nv, st));
            }
            launch_mg_twin(st, L.view(), L.inv_d.p, L.own ? L.vals32.p : nullptr, L.inv_d32.p, M.bad.p + 1 + l);
        }
        converted = true;
    }
    const MgLevel &L0 = *M.levels[0];
    if (!L0.own) {
        const bool half = spmv_layout == SpmvLayout::Sym;
        if (half) refresh_values(SpmvLayout::Sym);
        OGL_TRY(fp32_dev.ensure(half, pat_id, half ? sym_dev.map.n : d_vals.n, st));
        if (fp32_dev.epoch != vals_epoch || vals_epoch == 0) {
            if (!converted) OGL_HIP_CHECK(hipMemsetAsync(M.bad.p, 0x7f, sizeof(int32_t), st));
            fp32_dev.refresh(half ? sym_dev.map.p : nullptr, d_vals.p, M.bad.p, st);
            fp32_dev.epoch = vals_epoch;
            converted = true;
        }
    }
    if (!converted) return OGL_OK;
    std::vector<int32_t> bad((size_t)nl + 1);
    OGL_HIP_CHECK(hipMemcpyAsync(bad.data(), M.bad.p, bad.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    for (int l = 0; l <= nl; ++l) {  // (the fine level's coefficients first, then level by level)
        if (bad[(size_t)l] == MG_NONE_BAD) continue;
        int64_t row = bad[(size_t)l];
        if (l == 0) {
            fp32_dev.epoch = 0;
            OGL_TRY(fp32_bad_row(bad[0], &row));
            row = std::max<int64_t>(0, std::min<int64_t>(row, (int64_t)pat.n_rows - 1));
        }
        M.twin_of = 0;
        return fail(OGL_ERR_INVALID,
                    "preconditioner Multigrid: cyclePrecision single: a coefficient or the inverse diagonal of row %lld of "
                    "level %d%s is finite in double precision and not in single precision",
                    (long long)row, l == 0 ? 0 : l - 1, l <= 1 ? " (caller's numbering)" : "");
    }
    M.twin_of = M.generated;
    return OGL_OK;
}

int ogl_solver::generate_multigrid(PrecondData &P)
{
    hipStream_t st = reg->stream;
    const int max_levels = (int)prop("maxLevels", 9.0);
    const int32_t min_coarse = (int32_t)prop("minCoarseRows", 10.0);
    const bool hashed = prop("aggregation", 0.0) == 1.0;
    const int max_passes = (int)prop("aggregatePasses", 1.0);
    MultigridPart &M = P.mg;
    M.cg_iters = (int)prop("coarseSolverIters", 4.0);
    OGL_TRY(grow(M.scal, 1, st));
    OGL_TRY(grow(M.left, 1, st));
    if (M.levels.empty()) M.levels.emplace_back(new MgLevel);
    const DevCsr A0 = csr(false);
    MgCsr cur;
    cur.n = pat.n_rows;
    cur.nnz = pat.local_nnz;
    cur.row_ptrs = A0.row_ptrs;
    cur.cols = A0.cols;
    cur.vals = A0.vals;
    MgLevel &L0 = *M.levels[0];
    L0.own = pat.renumbered();
    if (L0.own) {
        // the hierarchy is that of the CALLER's numbering: level 0 = the device copy carried back through the permutation
        // (pattern and value map once per pattern on the host, the values gathered on the device per generation)
        if (!P.has_structure(pat_id, PrecondKind::Multigrid, 0)) {
            P.struct_pat_id = 0;
            OGL_TRY(download_local_pattern(pat));
            const int32_t N = pat.n_rows;
            std::vector<int32_t> rp((size_t)N + 1, 0), cc, map;
            cc.reserve((size_t)pat.local_nnz);
            map.reserve((size_t)pat.local_nnz);
            std::vector<std::pair<int32_t, int32_t>> ent;  // (caller column, device CSR position)
            for (int32_t i = 0; i < N; ++i) {
                const int32_t r = pat.new_id[(size_t)i];
                ent.clear();
                for (int32_t k = pat.row_ptrs[(size_t)r]; k < pat.row_ptrs[(size_t)r + 1]; ++k)
                    ent.emplace_back(pat.old_of[(size_t)pat.cols[(size_t)k]], k);
                std::stable_sort(ent.begin(), ent.end(), [](const std::pair<int32_t, int32_t> &a,
                                                            const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
                for (const auto &e : ent) {
                    cc.push_back(e.first);
                    map.push_back(e.second);
                }
                rp[(size_t)i + 1] = (int32_t)cc.size();
            }
            OGL_TRY(grow(L0.row_ptrs, rp.size(), st));
            OGL_TRY(grow(L0.cols, cc.size(), st));
            OGL_TRY(grow(M.map0, map.size(), st));
            OGL_TRY(reg->stager.h2d(L0.row_ptrs.p, rp.data(), rp.size() * sizeof(int32_t), st));
            if (!cc.empty()) {
                OGL_TRY(reg->stager.h2d(L0.cols.p, cc.data(), cc.size() * sizeof(int32_t), st));
                OGL_TRY(reg->stager.h2d(M.map0.p, map.data(), map.size() * sizeof(int32_t), st));
            }
            P.set_structure(pat_id, PrecondKind::Multigrid, 0);
        }
        OGL_TRY(grow(L0.vals, (size_t)cur.nnz, st));
        OGL_TRY(grow(M.in, (size_t)cur.n + 2, st));
        OGL_TRY(grow(M.out, (size_t)cur.n + 2, st));
        launch_gather_coeffs(st, cur.nnz, M.map0.p, A0.vals, L0.vals.p);
        cur.row_ptrs = L0.row_ptrs.p;
        cur.cols = L0.cols.p;
        cur.vals = L0.vals.p;
    } else if (P.struct_kind == PrecondKind::Multigrid) {
        P.struct_pat_id = 0;
    }
    int l = 0;
    for (;; ++l) {
        MgLevel &L = *M.levels[(size_t)l];
        const int32_t n = cur.n, m = cur.nnz;
        L.n = n;
        L.nnz = m;
        L.n_coarse = 0;
        OGL_TRY(grow(L.inv_d, (size_t)n + 2, st));
        OGL_TRY(grow(M.diag, (size_t)n, st));
        for (DevBuf<double> *v : {&L.xa, &L.xb, &L.t}) OGL_TRY(grow(*v, (size_t)n + 2, st));
        L.passes = 0;
        launch_mg_diag(st, cur, M.diag.p, L.inv_d.p);
        if (l >= max_levels || n <= min_coarse || n < 2) break;
        // (every work buffer at the size of the level's first pass: the later passes' matrices are smaller)
        OGL_TRY(grow(L.agg, (size_t)n, st));
        for (DevBuf<int32_t> *v : {&M.s, &M.flag, &M.incl, &M.cidx, &M.rows, &M.sorted, &L.agg_rows})
            OGL_TRY(grow(*v, (size_t)std::max(n, m), st));
        const size_t temp_bytes = mg_temp_bytes(n, m);
        OGL_TRY(grow(M.temp, temp_bytes, st));
        OGL_TRY(grow(M.keys, (size_t)m, st));
        OGL_TRY(grow(M.keys_sorted, (size_t)m, st));
        OGL_TRY(grow(M.vals_sorted, (size_t)m, st));
        if (M.levels.size() < (size_t)l + 2) M.levels.emplace_back(new MgLevel);
        MgLevel &C = *M.levels[(size_t)l + 1];
        // ---- up to aggregatePasses pairwise coarsenings, each of the matrix the one before it made; L.agg: their
        //      composition ----
        MgCsr pa = cur;         // the matrix of this pass
        bool in_place = false;  // pa is C's own arrays already
        for (int pass = 0; pass < max_passes; ++pass) {
            const int32_t pn = pa.n, pm = pa.nnz;
            if (pass > 0) {
                OGL_TRY(grow(M.pass_agg, (size_t)pn, st));
                launch_mg_diag(st, pa, M.diag.p, nullptr);
            }
            int32_t *const agg = pass == 0 ? L.agg.p : M.pass_agg.p;
            // ---- aggregation: up to MG_ROUNDS matching rounds, then the leftovers ----
            OGL_HIP_CHECK(hipMemsetAsync(agg, 0xff, (size_t)pn * sizeof(int32_t), st));
            int32_t prev_left = pn;
            for (int round = 0; round < MG_ROUNDS; ++round) {
                OGL_HIP_CHECK(hipMemsetAsync(M.left.p, 0, sizeof(int32_t), st));
                launch_mg_strongest(st, pa, M.diag.p, agg, 0, hashed, M.s.p);
                launch_mg_match(st, pn, M.s.p, agg, M.left.p);
                int32_t left = 0;
                OGL_TRY(read_i32(M.left.p, &left, st));
                if (left == 0 || left == prev_left || (double)left < 0.05 * (double)pn) break;
                prev_left = left;
            }
            launch_mg_strongest(st, pa, M.diag.p, agg, 1, hashed, M.s.p);
            launch_mg_join(st, pn, M.s.p, agg);
            // ---- numbering: roots in ascending order ----
            launch_mg_root_flag(st, pn, agg, M.flag.p);
            OGL_HIP_CHECK(mg_inclusive_sum(st, M.temp.p, temp_bytes, M.flag.p, M.incl.p, pn));
            int32_t nc = 0;
            OGL_TRY(read_i32(M.incl.p + (pn - 1), &nc, st));
            if (nc >= pn) break;  // (a pass that does not shrink is dropped and ends the level's passes)
            launch_mg_coarse_index(st, pn, agg, M.incl.p, M.cidx.p, M.rows.p);
            if (pass == 0)
                OGL_HIP_CHECK(hipMemcpyAsync(L.agg.p, M.cidx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            else
                launch_mg_compose(st, n, M.cidx.p, L.agg.p);
            // ---- A_c: stable sort of the entries by (agg(i), agg(j)), one entry per run, summed in sorted order ----
            launch_mg_keys(st, pa, M.cidx.p, M.keys.p);
            OGL_HIP_CHECK(mg_sort_entries(st, M.temp.p, temp_bytes, M.keys.p, M.keys_sorted.p, pa.vals, M.vals_sorted.p, pm));
            launch_mg_head_flag(st, pm, M.keys_sorted.p, M.flag.p);
            OGL_HIP_CHECK(mg_inclusive_sum(st, M.temp.p, temp_bytes, M.flag.p, M.incl.p, pm));
            int32_t mc = 0;
            OGL_TRY(read_i32(M.incl.p + (pm - 1), &mc, st));
            // (the level's last pass writes the kept level's own arrays; one that may be followed by another, scratch)
            in_place = pass + 1 == max_passes || nc <= min_coarse || nc < 2;
            MgCsr out;
            out.n = nc;
            out.nnz = mc;
            if (in_place) {
                OGL_TRY(grow(C.row_ptrs, (size_t)nc + 1, st));
                OGL_TRY(grow(C.cols, (size_t)mc, st));
                OGL_TRY(grow(C.vals, (size_t)mc, st));
                launch_mg_compact(st, pm, nc, M.keys_sorted.p, M.vals_sorted.p, M.incl.p, C.row_ptrs.p, C.cols.p, C.vals.p);
                out.row_ptrs = C.row_ptrs.p;
                out.cols = C.cols.p;
                out.vals = C.vals.p;
            } else {
                DevBuf<int32_t> &rp = M.pass_row_ptrs[pass & 1], &cc = M.pass_cols[pass & 1];
                DevBuf<double> &vv = M.pass_vals[pass & 1];
                OGL_TRY(grow(rp, (size_t)nc + 1, st));
                OGL_TRY(grow(cc, (size_t)mc, st));
                OGL_TRY(grow(vv, (size_t)mc, st));
                launch_mg_compact(st, pm, nc, M.keys_sorted.p, M.vals_sorted.p, M.incl.p, rp.p, cc.p, vv.p);
                out.row_ptrs = rp.p;
                out.cols = cc.p;
                out.vals = vv.p;
            }
            pa = out;
            ++L.passes;
            if (in_place) break;
        }
        if (L.passes == 0) break;  // (the first pass did not shrink: the hierarchy ends here)
        const int32_t nc = pa.n, mc = pa.nnz;
        if (!in_place) {  // (a later pass was dropped: the kept matrix is the scratch one of the pass before it)
            OGL_TRY(grow(C.row_ptrs, (size_t)nc + 1, st));
            OGL_TRY(grow(C.cols, (size_t)mc, st));
            OGL_TRY(grow(C.vals, (size_t)mc, st));
            OGL_HIP_CHECK(hipMemcpyAsync(C.row_ptrs.p, pa.row_ptrs, ((size_t)nc + 1) * sizeof(int32_t),
                                         hipMemcpyDeviceToDevice, st));
            if (mc > 0) {
                OGL_HIP_CHECK(hipMemcpyAsync(C.cols.p, pa.cols, (size_t)mc * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                OGL_HIP_CHECK(hipMemcpyAsync(C.vals.p, pa.vals, (size_t)mc * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
        }
        // ---- the members of every coarse row, ascending (rows[i] = i: k_mg_coarse_index of the first pass) ----
        OGL_TRY(grow(L.agg_ptr, (size_t)nc + 1, st));
        OGL_HIP_CHECK(mg_sort_rows(st, M.temp.p, temp_bytes, L.agg.p, M.sorted.p, M.rows.p, L.agg_rows.p, n));
        launch_mg_member_ptr(st, n, nc, M.sorted.p, L.agg_ptr.p);
        OGL_TRY(grow(C.b, (size_t)nc + 2, st));
        L.n_coarse = nc;
        C.n = nc;
        C.nnz = mc;
        cur = C.view();
    }
    M.n_levels = l + 1;
    MgLevel &last = *M.levels[(size_t)l];
    OGL_TRY(grow(last.r, (size_t)last.n + 2, st));
    OGL_TRY(grow(last.p, (size_t)last.n + 2, st));
    OGL_TRY(grow(last.part, n_chunks(last.n) + 1, st));
    // what the hierarchy looks like (mgLevels counts the matrices, the fine one included)
    props["mgLevels"] = (double)M.n_levels;
    double total = 0.0;
    for (int k = 0; k < M.n_levels; ++k) {
        props["mgRows" + std::to_string(k)] = (double)M.levels[(size_t)k]->n;
        props["mgNnz" + std::to_string(k)] = (double)M.levels[(size_t)k]->nnz;
        total += (double)M.levels[(size_t)k]->nnz;
        // (passes that made level k + 1; read-only)
        if (k + 1 < M.n_levels) props["mgPasses" + std::to_string(k)] = (double)M.levels[(size_t)k]->passes;
    }
    props["mgOperatorComplexity"] = M.levels[0]->nnz > 0 ? total / (double)M.levels[0]->nnz : 1.0;
    ++M.generated;  // (the levels' binary32 twin, if there is one, is that of the generation before)
    return OGL_OK;
}

void ogl_solver::mg_product(int level, const double *x, double *y, const DevScalars *gate)
{
    if (!precond_data->mg.levels[(size_t)level]->own)
        spmv_on(spmv_layout, SPMV_PLAIN, x, nullptr, y, SpmvDots{}, gate);
    else
        launch_mg_csr_spmv(reg->stream, precond_data->mg.levels[(size_t)level]->view(), x, y, gate);
}

// One visit of `level`: x = the cycle's answer to A_level x = b -- from x = 0, or (continued; never level 0 or the coarsest)
// from the answer of the visit before, which x then holds.  x is the level's own xb for every level but 0, so a continued
// visit reads it before the visit's last sweep writes it.  The level's b is not written by its own visits.
void ogl_solver::mg_cycle(int level, const double *b, double *x, const DevScalars *gate, int &launches, bool continued)
{
    hipStream_t st = reg->stream;
    const MultigridPart &M = precond_data->mg;
    const MgLevel &L = *M.levels[(size_t)level];
    const int32_t n = L.n;
    if (level >= mg_tail_first) {
        // this level and everything below it: one single-workgroup kernel (kernels_mg.hip, k_mg_tail)
        MgTail T;
        T.count = M.n_levels - level;
        T.cg_iters = M.cg_iters;
        T.coarse_visits = mg_coarse_visits;
        T.continued = continued ? 1 : 0;
        T.sweeps = mg_sweeps;
        T.scale = mg_scale;
        for (int k = 0; k < T.count; ++k) {
            const MgLevel &S = *M.levels[(size_t)(level + k)];
            MgTailLevel &D = T.lev[k];
            MgCsr A = S.view();
            if (!S.own) {  // (level 0 in the caller's numbering: the system matrix's own CSR arrays)
                const DevCsr A0 = csr(false);
                A.row_ptrs = A0.row_ptrs;
                A.cols = A0.cols;
                A.vals = A0.vals;
            }
            D.n = S.n;
            D.n_coarse = S.n_coarse;
            D.row_ptrs = A.row_ptrs;
            D.cols = A.cols;
            D.vals = A.vals;
            D.inv_d = S.inv_d.p;
            D.agg = S.agg.p;
            D.agg_ptr = S.agg_ptr.p;
            D.agg_rows = S.agg_rows.p;
            D.b = S.b.p;
            D.xa = S.xa.p;
            D.xb = S.xb.p;
            D.t = S.t.p;
            D.r = S.r.p;
            D.p = S.p.p;
            D.part = S.part.p;
        }
        launch_mg_tail(st, T, b, x, gate);
        ++launches;
        return;
    }
    if (level == M.n_levels - 1) {
        // the coarsest solver: coarseSolverIters iterations of unpreconditioned CG, no criterion; dots in the loop's tree
        MgScalars *sc = M.scal.p;
        const int n_part = (int)n_chunks(n);
        launch_mg_cg_init(st, n, b, L.r.p, x, L.p.p, gate);
        ++launches;
        for (int it = 0; it < M.cg_iters; ++it) {
            launch_partials_dot(st, n, L.r.p, L.r.p, L.part.p, gate);
            launch_mg_cg_fin(st, L.part.p, n_part, 0, it == 0, sc, gate);
            launch_mg_cg_step1(st, n, L.p.p, L.r.p, sc, gate);
            mg_product(level, L.p.p, L.t.p, gate);
            launch_partials_dot(st, n, L.p.p, L.t.p, L.part.p, gate);
            launch_mg_cg_fin(st, L.part.p, n_part, 1, 0, sc, gate);
            launch_mg_cg_step2(st, n, x, L.r.p, L.p.p, L.t.p, sc, gate);
            launches += 7;
        }
        return;
    }
    const MgLevel &C = *M.levels[(size_t)level + 1];
    const MgCsr A = L.view();
    // smootherSweeps pre-sweeps (the first from x = 0: no product; of a continued visit: a full sweep from x), residual and
    // restriction.  x ping-pongs between xa and xb (no sweep writes the vector it reads): the first pre-sweep writes xa, so
    // `cur`, what the last one wrote and the restriction reads, is xa for an odd count and xb for an even one.
    const int nu = mg_sweeps;
    const double scale = mg_scale;
    double *cur = L.xa.p;
    const auto other = [&L](const double *v) { return v == L.xa.p ? L.xb.p : L.xa.p; };
    if (continued)
        launch_mg_csr_sweep(st, A, L.inv_d.p, b, x, nullptr, nullptr, scale, cur, gate);
    else
        launch_mg_jacobi0(st, n, b, L.inv_d.p, cur, gate);
    ++launches;
    const bool layout = !L.own;  // (level 0 in the caller's numbering: products on the in-loop layout, sweeps behind them)
    if (layout) {
        for (int k = 1; k < nu; ++k, cur = other(cur)) {
            mg_product(0, cur, L.t.p, gate);
            launch_mg_sweep_epi(st, n, b, L.t.p, L.inv_d.p, cur, other(cur), gate);
            launches += 2;
        }
        mg_product(0, cur, L.t.p, gate);
        launch_mg_restrict(st, C.n, L.agg_ptr.p, L.agg_rows.p, A, b, cur, L.t.p, C.b.p, gate);
        launches += 2;
    } else {
        for (int k = 1; k < nu; ++k, cur = other(cur)) {
            launch_mg_csr_sweep(st, A, L.inv_d.p, b, cur, nullptr, nullptr, scale, other(cur), gate);
            ++launches;
        }
        launch_mg_restrict(st, C.n, L.agg_ptr.p, L.agg_rows.p, A, b, cur, nullptr, C.b.p, gate);
        ++launches;
    }
    // the coarse correction lands in the coarse level's xb (its last post-sweep writes there; the coarsest CG too); the
    // visits after the first continue from there with the same C.b
    mg_cycle(level + 1, C.b.p, C.xb.p, gate, launches, false);
    if (level + 2 < M.n_levels)
        for (int visit = 1; visit < mg_coarse_visits; ++visit) mg_cycle(level + 1, C.b.p, C.xb.p, gate, launches, true);
    // the scaled correction and smootherSweeps post-sweeps, the last of them into x (level 0: the caller's vector; below
    // it the level's xb, where the alternation lands whatever the count)
    if (layout) {
        launch_mg_prolong(st, n, cur, C.xb.p, L.agg.p, scale, other(cur), gate);
        cur = other(cur);
        ++launches;
        for (int k = 0; k < nu; ++k, cur = other(cur)) {
            mg_product(0, cur, L.t.p, gate);
            launch_mg_sweep_epi(st, n, b, L.t.p, L.inv_d.p, cur, k == nu - 1 ? x : other(cur), gate);
            launches += 2;
        }
    } else {
        // (the prolongation folded into the first post-sweep: t_j = x_j + scale x_c[agg(j)], product and sum rounded once each)
        for (int k = 0; k < nu; ++k, cur = other(cur)) {
            if (k == 0)
                launch_mg_csr_sweep(st, A, L.inv_d.p, b, cur, C.xb.p, L.agg.p, scale, k == nu - 1 ? x : other(cur), gate);
            else
                launch_mg_csr_sweep(st, A, L.inv_d.p, b, cur, nullptr, nullptr, scale, k == nu - 1 ? x : other(cur), gate);
            ++launches;
        }
    }
}

// Level 0's product in single precision with its epilogue (kernels_mixed.hip): on the fp32 twin of the half storage's
// planes where that is the in-loop layout, else on the fp32 value array beside the device CSR.
void ogl_solver::mg_fine32(MxEpilogue epi, const float *x, const MgEpi &e)
{
    if (fp32_dev.half)
        launch_mg_fine_sym(reg->stream, sym(), fp32_dev.planes.p, epi, x, e);
    else
        launch_mg_fine_csr(reg->stream, csr(false), fp32_dev.vals.p, epi, x, e);
}

// mg_cycle on binary32 operands (cyclePrecision single): the same steps in the same order on the levels' twin and fp32
// vectors.  Level 0 (in64 != nullptr) reads the fp64 residual in64 -- b = fl32(in64) is formed by its first pre-sweep -- and
// its last post-sweep writes out64 as doubles; its products, where it is the system matrix in the in-loop layout, carry
// the sweep or the residual as their epilogue, so no elementwise pass follows a product.
void ogl_solver::mg_cycle32(int level, const float *b, float *x, const double *in64, double *out64, const DevScalars *gate,
                            int &launches, bool continued)
{
    hipStream_t st = reg->stream;
    const MultigridPart &M = precond_data->mg;
    MgLevel &L = *M.levels[(size_t)level];
    const int32_t n = L.n;
    if (level >= mg_tail_first) {  // (never level 0: apply_multigrid)
        MgTail32 T;
        T.count = M.n_levels - level;
        T.cg_iters = M.cg_iters;
        T.coarse_visits = mg_coarse_visits;
        T.continued = continued ? 1 : 0;
        T.sweeps = mg_sweeps;
        T.scale = mg_scale;
        for (int k = 0; k < T.count; ++k) {
            const MgLevel &S = *M.levels[(size_t)(level + k)];
            MgTailLevelOf<float> &D = T.lev[k];
            D.n = S.n;
            D.n_coarse = S.n_coarse;
            D.row_ptrs = S.row_ptrs.p;
            D.cols = S.cols.p;
            D.vals = S.vals32.p;
            D.inv_d = S.inv_d32.p;
            D.agg = S.agg.p;
            D.agg_ptr = S.agg_ptr.p;
            D.agg_rows = S.agg_rows.p;
            D.b = S.b32.p;
            D.xa = S.xa32.p;
            D.xb = S.xb32.p;
            D.t = S.t32.p;
            D.r = S.r32.p;
            D.p = S.p32.p;
            D.part = S.part.p;
        }
        launch_mg_tail(st, T, b, x, gate);
        ++launches;
        return;
    }
    const bool fine = in64 && !L.own;  // level 0 as the system matrix in the in-loop layout
    MgEpi e;
    e.b = b;
    e.inv_d = L.inv_d32.p;
    e.gate = gate;
    if (level == M.n_levels - 1) {
        // the coarsest solver; its sums are wide (fp64 products of the casts) in the loop's tree
        MgScalars *sc = M.scal.p;
        const int n_part = (int)n_chunks(n);
        launch_mg_cg_init(st, n, b, in64, L.r32.p, x, L.p32.p, gate);
        ++launches;
        for (int it = 0; it < M.cg_iters; ++it) {
            launch_mg_wide_dot(st, n, L.r32.p, L.r32.p, L.part.p, gate);
            launch_mg_cg_fin(st, L.part.p, n_part, 0, it == 0, sc, gate);
            launch_mg_cg_step1(st, n, L.p32.p, L.r32.p, sc, gate);
            if (fine) {
                e.out = L.t32.p;
                mg_fine32(MX_EPI_PLAIN, L.p32.p, e);
            } else {
                launch_mg_csr_spmv(st, L.view32(), L.p32.p, L.t32.p, gate);
            }
            launch_mg_wide_dot(st, n, L.p32.p, L.t32.p, L.part.p, gate);
            launch_mg_cg_fin(st, L.part.p, n_part, 1, 0, sc, gate);
            launch_mg_cg_step2(st, n, x, L.r32.p, L.p32.p, L.t32.p, sc, gate);
            launches += 7;
        }
        if (in64) {  // (a hierarchy of one level)
            launch_mg_widen(st, n, x, out64, gate);
            ++launches;
        }
        return;
    }
    MgLevel &C = *M.levels[(size_t)level + 1];
    const MgCsr32 A = L.view32();
    // smootherSweeps pre-sweeps, residual and restriction; the buffers by parity as in mg_cycle
    const int nu = mg_sweeps;
    const float scale = (float)mg_scale;  // (fl32 of the keyword's value)
    float *cur = L.xa32.p;
    const auto other = [&L](const float *v) { return v == L.xa32.p ? L.xb32.p : L.xa32.p; };
    if (in64)
        launch_mg_jacobi0_in(st, n, in64, L.inv_d32.p, L.b32.p, cur, gate);
    else if (continued)
        launch_mg_csr_sweep(st, A, L.inv_d32.p, b, x, nullptr, nullptr, scale, cur, nullptr, gate);
    else
        launch_mg_jacobi0(st, n, b, L.inv_d32.p, cur, gate);
    ++launches;
    if (fine) {
        for (int k = 1; k < nu; ++k, cur = other(cur)) {
            e.out = other(cur);
            mg_fine32(MX_EPI_SWEEP, cur, e);
            ++launches;
        }
        e.out = L.t32.p;
        mg_fine32(MX_EPI_RESIDUAL, cur, e);
        launch_mg_restrict(st, C.n, L.agg_ptr.p, L.agg_rows.p, A, b, cur, L.t32.p, C.b32.p, gate);
        launches += 2;
    } else {
        for (int k = 1; k < nu; ++k, cur = other(cur)) {
            launch_mg_csr_sweep(st, A, L.inv_d32.p, b, cur, nullptr, nullptr, scale, other(cur), nullptr, gate);
            ++launches;
        }
        launch_mg_restrict(st, C.n, L.agg_ptr.p, L.agg_rows.p, A, b, cur, nullptr, C.b32.p, gate);
        ++launches;
    }
    mg_cycle32(level + 1, C.b32.p, C.xb32.p, nullptr, nullptr, gate, launches, false);
    if (level + 2 < M.n_levels)
        for (int visit = 1; visit < mg_coarse_visits; ++visit)
            mg_cycle32(level + 1, C.b32.p, C.xb32.p, nullptr, nullptr, gate, launches, true);
    // the scaled correction and smootherSweeps post-sweeps; the last of them writes x, or (level 0) out64 as doubles
    if (fine) {
        launch_mg_prolong(st, n, cur, C.xb32.p, L.agg.p, scale, other(cur), gate);
        cur = other(cur);
        ++launches;
        for (int k = 0; k < nu; ++k, cur = other(cur)) {
            const bool end = k == nu - 1;
            e.out = end ? nullptr : other(cur);
            e.out64 = end ? out64 : nullptr;
            mg_fine32(end ? MX_EPI_SWEEP64 : MX_EPI_SWEEP, cur, e);
            ++launches;
        }
    } else {
        for (int k = 0; k < nu; ++k, cur = other(cur)) {
            const bool end = k == nu - 1;
            float *const dst = end ? (in64 ? nullptr : x) : other(cur);
            launch_mg_csr_sweep(st, A, L.inv_d32.p, b, cur, k == 0 ? C.xb32.p : nullptr, k == 0 ? L.agg.p : nullptr, scale, dst,
                                end ? out64 : nullptr, gate);
            ++launches;
        }
    }
}

void ogl_solver::apply_multigrid(const double *in, double *out, const DevScalars *gate, double *dot_part)
{
    int launches = 0;
    const MultigridPart &M = precond_data->mg;
    // the tail: the levels of at most mgTailRows rows (this solver's own property, also on a stored hierarchy); never
    // more than the kernel's level table and reduction tree hold
    const double tail_rows = std::min(prop("mgTailRows", (double)MG_TAIL_DEFAULT_ROWS), (double)MG_TAIL_MAX_ROWS);
    mg_tail_first = M.n_levels;
    while (mg_tail_first > 0 && M.n_levels - mg_tail_first < MG_TAIL_MAX_LEVELS &&
           (double)M.levels[(size_t)mg_tail_first - 1]->n <= tail_rows)
        --mg_tail_first;
    // (single precision: level 0 arrives and leaves in fp64 and takes its products from the in-loop layout's fp32 copy --
    //  it is launched, whatever its size)
    if (mg_single && mg_tail_first < 1) mg_tail_first = 1;
    props["mgTailLevels"] = (double)(M.n_levels - mg_tail_first);
    props["mgTailRows"] = tail_rows;
    if (mg_single) {
        MgLevel &L0 = *M.levels[0];
        if (pat.renumbered()) {
            launch_factor_gather_perm(reg->stream, pat.n_rows, d_new_id.p, in, M.in.p, gate);
            mg_cycle32(0, L0.b32.p, L0.xb32.p, M.in.p, M.out.p, gate, launches, false);
            launch_factor_scatter_perm(reg->stream, pat.n_rows, d_new_id.p, M.out.p, out, gate);
            launches += 2;
        } else {
            mg_cycle32(0, L0.b32.p, L0.xb32.p, in, out, gate, launches, false);
        }
    } else if (pat.renumbered()) {  // (the vectors carried into the caller's order and back, as apply_factor does)
        launch_factor_gather_perm(reg->stream, pat.n_rows, d_new_id.p, in, M.in.p, gate);
        mg_cycle(0, M.in.p, M.out.p, gate, launches, false);
        launch_factor_scatter_perm(reg->stream, pat.n_rows, d_new_id.p, M.out.p, out, gate);
        launches += 2;
    } else {
        mg_cycle(0, in, out, gate, launches, false);
    }
    props["mgLaunchesPerApply"] = (double)launches;  // (without the fused dot of a Krylov turn)
    if (dot_part) launch_partials_dot(reg->stream, pat.n_rows, in, out, dot_part, gate);
}

// ------------------------------------------------------------------------------------------
// the hierarchy handed out (tests, diagnostics)
// ------------------------------------------------------------------------------------------
static int mg_current(ogl_solver *s, int32_t level, const char *who)
{
    if (!s) return fail(OGL_ERR_INVALID, "NULL solver");
    if (!s->matrix_set || !s->precond_ready || !s->precond_current() || !s->precond_data || !s->precond_data->multigrid())
        return fail(OGL_ERR_STATE, "%s: no current Multigrid hierarchy (none was set up by the last solve, another field "
                                   "regenerated the shared one, or the pattern changed): solve again first", who);
    if (level < 0 || level >= s->precond_data->mg.n_levels)
        return fail(OGL_ERR_INVALID, "%s: level %d outside [0, %d)", who, level, s->precond_data->mg.n_levels);
    return OGL_OK;
}

extern "C" int ogl_solver_mg_level_dims(ogl_solver *s, int32_t level, ogl_label *rows, ogl_label *nnz)
{
    OGL_TRY(mg_current(s, level, "ogl_solver_mg_level_dims"));
    const MgLevel &L = *s->precond_data->mg.levels[(size_t)level];
    if (rows) *rows = L.n;
    if (nnz) *nnz = L.nnz;
    return OGL_OK;
}

extern "C" int ogl_solver_get_mg_level(ogl_solver *s, int32_t level, ogl_label *row_ptrs, ogl_label *cols, ogl_scalar *vals,
                                       ogl_label *agg)
{
    try {
        OGL_TRY(mg_current(s, level, "ogl_solver_get_mg_level"));
        OGL_HIP_CHECK(hipSetDevice(s->reg->device));
        hipStream_t st = s->reg->stream;
        const MgLevel &L = *s->precond_data->mg.levels[(size_t)level];
        MgCsr A = L.view();
        if (!L.own) {
            const DevCsr A0 = s->csr(false);
            A.row_ptrs = A0.row_ptrs;
            A.cols = A0.cols;
            A.vals = A0.vals;
        }
        Stager &sg = s->reg->stager;
        if (row_ptrs) OGL_TRY(sg.d2h(row_ptrs, A.row_ptrs, ((size_t)L.n + 1) * sizeof(int32_t), st));
        if (cols && L.nnz > 0) OGL_TRY(sg.d2h(cols, A.cols, (size_t)L.nnz * sizeof(int32_t), st));
        if (vals && L.nnz > 0) OGL_TRY(sg.d2h(vals, A.vals, (size_t)L.nnz * sizeof(double), st));
        if (agg) {
            if (L.n_coarse == 0) return fail(OGL_ERR_INVALID, "ogl_solver_get_mg_level: the coarsest level has no aggregates");
            OGL_TRY(sg.d2h(agg, L.agg.p, (size_t)L.n * sizeof(int32_t), st));
        }
        return OGL_OK;
    } catch (const std::exception &e) {
        return fail(OGL_ERR_INVALID, "exception: %s", e.what());
    }
}
