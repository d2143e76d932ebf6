// solver_mg.cpp -- preconditioner Multigrid (Preconditioner.H:259-341): generation of the aggregation hierarchy on the
// device in named steps (level 0 in the caller's numbering, one aggregation pass, one Galerkin product), one V-cycle as the
// apply, and the entry points that hand the hierarchy out.  The cycle is ONE body, mg_cycle<T>, for both operand types
// (coarseVisits > 1: every coarse level but the coarsest visited that often per visit of its parent; cyclePrecision single:
// T = float; smootherSweeps sweeps before and after the coarse correction, which is scaled by correctionScale); what the two
// precisions do differently at level 0 is in the overloads in front of it.  Kernels: kernels_mg.hip; the contract:
// DESIGN.md section 7b.
#include "solver_internal.hpp"

#include <algorithm>
#include <cassert>
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

// (every device-to-host read of a generation goes through here and is counted: property mgGenerateHostReads)
int read_i32(MultigridPart &M, const int32_t *dev, int32_t *host, hipStream_t st)
{
    ++M.host_reads;
    OGL_HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    return OGL_OK;
}

}  // namespace

int ogl_solver::check_multigrid_keywords()
{
    // (the keywords of the preconditioner's sub-dictionary travel as properties, Preconditioner.H:297-317)
    if (knob<Knob::cycle>() != 0.0)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner Multigrid: cycle %s is not built (only cycle v)",
                    knob<Knob::cycle>() == 1.0 ? "w" : "f");
    if (knob<Knob::zeroGuess>() == 0.0)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner Multigrid: zeroGuess false is not built");
    if (knob<Knob::maxLevels>() < 0.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: maxLevels %d is negative", (int)knob<Knob::maxLevels>());
    if (knob<Knob::coarseSolverIters>() < 0.0)
        return fail(OGL_ERR_INVALID, "preconditioner Multigrid: coarseSolverIters %d is negative",
                    (int)knob<Knob::coarseSolverIters>());
    OGL_TRY(check_knob(Knob::aggregation));
    OGL_TRY(check_knob(Knob::aggregatePasses));
    OGL_TRY(check_knob(Knob::aggregateCaching));
    // (read-only: 1 once this solve's generation turns out to be a refresh -- not where a stored hierarchy is applied as it is)
    props["mgAggregatesReused"] = 0.0;
    OGL_TRY(check_knob(Knob::coarseVisits));
    OGL_TRY(check_knob(Knob::cyclePrecision));
    OGL_TRY(check_knob(Knob::smootherSweeps));
    // (a condition, not a tuning value: with an exact coarse solve the correction step I - scale Pi stops contracting at 2)
    return check_knob(Knob::correctionScale);
}

// This solver's side of an apply of the hierarchy (its own or a stored one): coarseVisits, and how often one apply then
// visits every level -- level 0 once, every level below it coarseVisits times per visit of its parent, the coarsest as
// often as its parent.  A hierarchy too deep for that many visits is refused here, before any apply.
int ogl_solver::prepare_multigrid_apply()
{
    const MultigridPart &M = precond_data->mg;
    mg_coarse_visits = (int)knob<Knob::coarseVisits>();
    set_knob<Knob::coarseVisits>((double)mg_coarse_visits);
    // smootherSweeps and correctionScale are the applier's too; check_multigrid_keywords has refused the rest, and an
    // apply never runs with a count the ping-pong of the sweeps was not built for
    OGL_TRY(check_knob(Knob::smootherSweeps));
    OGL_TRY(check_knob(Knob::correctionScale));
    mg_sweeps = (int)knob<Knob::smootherSweeps>();
    mg_scale = knob<Knob::correctionScale>();
    set_knob<Knob::smootherSweeps>((double)mg_sweeps);
    set_knob<Knob::correctionScale>(mg_scale);
    // (read-only, of the hierarchy in use: the maps kept for keyword aggregateCaching and the refreshes it has left)
    props["mgKeptBytes"] = (double)M.kept_bytes();
    props["mgAggregateCachingLeft"] = (double)(M.kept_for.valid ? M.kept_left : 0);
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
    mg_single = knob<Knob::cyclePrecision>() == 1.0;
    if (mg_single) OGL_TRY(prepare_multigrid_single());
    props["mgCyclePrecisionInUse"] = mg_single ? 1.0 : 0.0;
    return OGL_OK;
}

// cyclePrecision single ("the cycle in single precision"): what an apply on binary32 operands needs
// besides the hierarchy.  (1) The levels' float operands -- values and 1 / d rounded from the stored doubles by one kernel
// per level, and the levels' vectors -- once per generated hierarchy, whoever applies it.  (2) Where level 0 is the system
// matrix in the in-loop layout, the fp32 copy the mixed-precision mode uses (Fp32Dev), refreshed per values epoch.  A value
// that is finite in fp64 and not in binary32 fails the solve; what failed is left stale, so that the next solve converts --
// and reports -- again.
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
            MgOperands<float> &F = L.flt;
            const size_t nv = (size_t)L.n + 4;  // (a trailing pair access of the last odd row stays inside)
            OGL_TRY(grow(F.inv_d, nv, st));
            if (L.own) OGL_TRY(grow(F.vals, (size_t)L.nnz + 2, st));
            for (DevBuf<float> *v : {&F.b, &F.xa, &F.xb, &F.t}) OGL_TRY(grow(*v, nv, st));
            if (l == nl - 1) {
                OGL_TRY(grow(F.r, nv, st));
                OGL_TRY(grow(F.p, nv, st));
            }
            launch_mg_twin(st, L.view<double>(), L.dbl.inv_d.p, L.own ? F.vals.p : nullptr, F.inv_d.p, M.bad.p + 1 + l);
        }
        converted = true;
    }
    const MgLevel &L0 = *M.levels[0];
    if (!L0.own) {
        const bool half = spmv_layout == SpmvLayout::Sym;
        if (half) refresh_values(SpmvLayout::Sym);
        OGL_TRY(fp32_dev.ensure(half, pat_id, half ? sym_dev.map.n : d_vals.n, 0, st));  // (the cycle is the local block's)
        if (fp32_dev.epoch != vals_epoch || vals_epoch == 0) {
            if (!converted) OGL_HIP_CHECK(hipMemsetAsync(M.bad.p, 0x7f, sizeof(int32_t), st));
            fp32_dev.refresh(half ? sym_dev.map.p : nullptr, d_vals.p, nullptr, M.bad.p, st);
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

// The matrix a level really is.  Level 0 in the caller's numbering keeps none of its own: it is the system matrix's CSR
// arrays.
template <>
MgCsr ogl_solver::mg_matrix<double>(const MgLevel &L) const
{
    if (L.own) return L.view<double>();
    const DevCsr A0 = csr(false);
    return MgCsr{L.n, L.nnz, A0.row_ptrs, A0.cols, A0.vals};
}
// (In single precision such a level has no CSR matrix -- its products come from the in-loop layout's fp32 copy, mg_fine32 --
//  and what needs one, the tail, is never given level 0: apply_multigrid.)
template <>
MgCsrOf<float> ogl_solver::mg_matrix<float>(const MgLevel &L) const
{
    assert(L.own);
    return L.view<float>();
}

// ------------------------------------------------------------------------------------------
// generation
// ------------------------------------------------------------------------------------------
namespace {

// Where a Galerkin product is written: a kept level's own arrays, or the scratch arrays between two passes.
struct MgCsrBufs {
    DevBuf<int32_t> &row_ptrs, &cols;
    DevBuf<double> &vals;
    int reserve(int32_t n, int32_t nnz, hipStream_t st) const
    {
        OGL_TRY(grow(row_ptrs, (size_t)n + 1, st));
        OGL_TRY(grow(cols, (size_t)nnz, st));
        return grow(vals, (size_t)nnz, st);
    }
    MgCsr view(int32_t n, int32_t nnz) const { return MgCsr{n, nnz, row_ptrs.p, cols.p, vals.p}; }
    int copy_from(const MgCsr &A, hipStream_t st) const
    {
        OGL_TRY(reserve(A.n, A.nnz, st));
        OGL_HIP_CHECK(hipMemcpyAsync(row_ptrs.p, A.row_ptrs, ((size_t)A.n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        if (A.nnz > 0) {
            OGL_HIP_CHECK(hipMemcpyAsync(cols.p, A.cols, (size_t)A.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            OGL_HIP_CHECK(hipMemcpyAsync(vals.p, A.vals, (size_t)A.nnz * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        return OGL_OK;
    }
};

// One pairwise coarsening of A (its diagonal in M.diag) into `agg`: up to MG_ROUNDS matching rounds, the leftovers joined
// to their strongest aggregated neighbour, the roots numbered in ascending order.  *nc: the aggregates; where that is fewer
// than A's rows, M.cidx holds every row's coarse index (and M.rows the identity), else nothing shrank and the pass is void.
int mg_aggregate(hipStream_t st, MultigridPart &M, const MgCsr &A, bool hashed, size_t temp_bytes, int32_t *agg, int32_t *nc)
{
    const int32_t n = A.n;
    OGL_HIP_CHECK(hipMemsetAsync(agg, 0xff, (size_t)n * sizeof(int32_t), st));
    int32_t prev_left = n;
    for (int round = 0; round < MG_ROUNDS; ++round) {
        OGL_HIP_CHECK(hipMemsetAsync(M.left.p, 0, sizeof(int32_t), st));
        launch_mg_strongest(st, A, M.diag.p, agg, 0, hashed, M.s.p);
        launch_mg_match(st, n, M.s.p, agg, M.left.p);
        int32_t left = 0;
        OGL_TRY(read_i32(M, M.left.p, &left, st));
        if (left == 0 || left == prev_left || (double)left < 0.05 * (double)n) break;
        prev_left = left;
    }
    launch_mg_strongest(st, A, M.diag.p, agg, 1, hashed, M.s.p);
    launch_mg_join(st, n, M.s.p, agg);
    launch_mg_root_flag(st, n, agg, M.flag.p);
    OGL_HIP_CHECK(mg_inclusive_sum(st, M.temp.p, temp_bytes, M.flag.p, M.incl.p, n));
    OGL_TRY(read_i32(M, M.incl.p + (n - 1), nc, st));
    if (*nc < n) launch_mg_coarse_index(st, n, agg, M.incl.p, M.cidx.p, M.rows.p);
    return OGL_OK;
}

// A_c = the Galerkin product of A under the coarse indices in M.cidx (nc of them), into dst: a stable sort of the entries
// by (agg(i), agg(j)), one entry per run, summed in sorted order.  *out: A_c.  keep (keyword aggregateCaching): the level
// whose pass `pass` this is, to be left the maps of a later refresh -- the sort then carries every entry's position
// (the same stable sort of the same keys: the same order) and the values are gathered behind it; nullptr: today's launches.
int mg_galerkin(hipStream_t st, MultigridPart &M, const MgCsr A, int32_t nc, size_t temp_bytes, const MgCsrBufs &dst, MgCsr *out,
                MgLevel *keep, int pass)
{
    const int32_t m = A.nnz;
    launch_mg_keys(st, A, M.cidx.p, M.keys.p);
    if (keep) {
        DevBuf<int32_t> &src = keep->kept_src[pass];
        OGL_TRY(grow(src, (size_t)m, st));
        launch_mg_iota(st, m, M.sorted.p);  // (M.sorted: free until the level's member lists)
        OGL_HIP_CHECK(mg_sort_entry_index(st, M.temp.p, temp_bytes, M.keys.p, M.keys_sorted.p, M.sorted.p, src.p, m));
        launch_gather_coeffs(st, m, src.p, A.vals, M.vals_sorted.p);
    } else {
        OGL_HIP_CHECK(mg_sort_entries(st, M.temp.p, temp_bytes, M.keys.p, M.keys_sorted.p, A.vals, M.vals_sorted.p, m));
    }
    launch_mg_head_flag(st, m, M.keys_sorted.p, M.flag.p);
    OGL_HIP_CHECK(mg_inclusive_sum(st, M.temp.p, temp_bytes, M.flag.p, M.incl.p, m));
    int32_t mc = 0;
    OGL_TRY(read_i32(M, M.incl.p + (m - 1), &mc, st));
    OGL_TRY(dst.reserve(nc, mc, st));
    launch_mg_compact(st, m, nc, M.keys_sorted.p, M.vals_sorted.p, M.incl.p, dst.row_ptrs.p, dst.cols.p, dst.vals.p);
    if (keep) {
        OGL_TRY(grow(keep->kept_ptr[pass], (size_t)mc + 1, st));
        launch_mg_run_ptr(st, m, M.flag.p, M.incl.p, keep->kept_ptr[pass].p);
        keep->kept_nnz[pass] = mc;
    }
    *out = dst.view(nc, mc);
    return OGL_OK;
}

}  // namespace

// A renumbered device copy: the hierarchy is that of the CALLER's numbering, so level 0 is the device copy carried back
// through the permutation.  Here its pattern and the position of every entry in the device CSR (M.map0), once per pattern
// on the host; the values are gathered on the device per generation.
int ogl_solver::mg_caller_numbered_level0(PrecondData &P)
{
    if (P.has_structure(pat_id, PrecondKind::Multigrid, 0)) return OGL_OK;
    hipStream_t st = reg->stream;
    MultigridPart &M = P.mg;
    MgLevel &L0 = *M.levels[0];
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
    return OGL_OK;
}

// Keyword aggregateCaching N ("kept aggregates"): an object whose aggregates were made for what this
// solver asks for has its values refreshed under them, N times between two full generations.  Which object that is stays
// init_preconditioner's rule.
int ogl_solver::generate_multigrid(PrecondData &P)
{
    MultigridPart &M = P.mg;
    const int keep = (int)knob<Knob::aggregateCaching>();
    MultigridPart::KeptFor asking;
    asking.valid = true;
    asking.pat_id = pat_id;
    asking.rows = pat.n_rows;
    asking.nnz = pat.local_nnz;
    asking.own = pat.renumbered();
    asking.hashed = knob<Knob::aggregation>() == 1.0;
    asking.passes = (int)knob<Knob::aggregatePasses>();
    asking.max_levels = (int)knob<Knob::maxLevels>();
    asking.min_coarse = knob<Knob::minCoarseRows>();
    M.cg_iters = (int)knob<Knob::coarseSolverIters>();
    M.host_reads = 0;
    const bool refresh = keep > 0 && M.kept_left > 0 && M.kept_for == asking;
    if (refresh) {
        --M.kept_left;
        OGL_TRY(refresh_multigrid(P));
    } else {
        OGL_TRY(generate_multigrid_full(P, asking, keep));
    }
    publish_multigrid(M);
    props["mgAggregatesReused"] = refresh ? 1.0 : 0.0;
    props["mgGenerateHostReads"] = (double)M.host_reads;
    ++M.generated;  // (the levels' binary32 twin, if there is one, is that of the generation before)
    return OGL_OK;
}

// Only the values: level 0's through map0 on a renumbered device copy, every pass's from its source's through the kept
// maps -- the last pass of a level into the kept level, the ones before it into the scratch values the full generation used
// -- and 1 / d of every level.  Stream-ordered launches, nothing read back.
int ogl_solver::refresh_multigrid(PrecondData &P)
{
    hipStream_t st = reg->stream;
    MultigridPart &M = P.mg;
    MgLevel &L0 = *M.levels[0];
    if (L0.own) {
        OGL_TRY(mg_caller_numbered_level0(P));
        launch_gather_coeffs(st, L0.nnz, M.map0.p, csr(false).vals, L0.dbl.vals.p);
    }
    // (property mgKeepStream 1, measurements: the maps loaded past the caches)
    const bool stream = knob<Knob::mgKeepStream>() != 0.0;
    for (int l = 0; l < M.n_levels; ++l) {
        MgLevel &L = *M.levels[(size_t)l];
        const MgCsr A = mg_matrix<double>(L);
        launch_mg_diag(st, A, M.diag.p, L.dbl.inv_d.p);
        if (l + 1 == M.n_levels) break;
        MgLevel &C = *M.levels[(size_t)l + 1];
        const double *from = A.vals;
        for (int pass = 0; pass < L.passes; ++pass) {
            double *to = pass + 1 == L.passes ? C.dbl.vals.p : M.pass_vals[pass & 1].p;
            launch_mg_regalerkin(st, L.kept_nnz[pass], L.kept_ptr[pass].p, L.kept_src[pass].p, from, to, stream);
            from = to;
        }
    }
    return OGL_OK;
}

void ogl_solver::publish_multigrid(const MultigridPart &M)
{
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
}

// The record is invalid from the start of a full generation to its end, so one that fails half-way leaves nothing to
// reuse; keep == 0 keeps nothing and leaves it invalid.
int ogl_solver::generate_multigrid_full(PrecondData &P, const MultigridPart::KeptFor &asking, int keep)
{
    hipStream_t st = reg->stream;
    const int max_levels = asking.max_levels;
    const int32_t min_coarse = (int32_t)asking.min_coarse;
    const bool hashed = asking.hashed;
    const int max_passes = asking.passes;
    MultigridPart &M = P.mg;
    M.kept_for.valid = false;
    OGL_TRY(grow(M.scal, 1, st));
    OGL_TRY(grow(M.left, 1, st));
    if (M.levels.empty()) M.levels.emplace_back(new MgLevel);
    MgLevel &L0 = *M.levels[0];
    L0.n = pat.n_rows;
    L0.nnz = pat.local_nnz;
    L0.own = pat.renumbered();
    if (L0.own) {
        OGL_TRY(mg_caller_numbered_level0(P));
        OGL_TRY(grow(L0.dbl.vals, (size_t)L0.nnz, st));
        OGL_TRY(grow(M.in, (size_t)L0.n + 2, st));
        OGL_TRY(grow(M.out, (size_t)L0.n + 2, st));
        launch_gather_coeffs(st, L0.nnz, M.map0.p, csr(false).vals, L0.dbl.vals.p);
    } else if (P.struct_kind == PrecondKind::Multigrid) {
        P.struct_pat_id = 0;
    }
    MgCsr cur = mg_matrix<double>(L0);
    int l = 0;
    for (;; ++l) {
        MgLevel &L = *M.levels[(size_t)l];
        MgOperands<double> &V = L.dbl;
        const int32_t n = cur.n, m = cur.nnz;
        L.n = n;
        L.nnz = m;
        L.n_coarse = 0;
        OGL_TRY(grow(V.inv_d, (size_t)n + 2, st));
        OGL_TRY(grow(M.diag, (size_t)n, st));
        for (DevBuf<double> *v : {&V.xa, &V.xb, &V.t}) OGL_TRY(grow(*v, (size_t)n + 2, st));
        L.passes = 0;
        launch_mg_diag(st, cur, M.diag.p, V.inv_d.p);
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
        const MgCsrBufs kept{C.row_ptrs, C.cols, C.dbl.vals};
        // ---- up to aggregatePasses pairwise coarsenings, each of the matrix the one before it made; L.agg: their
        //      composition ----
        MgCsr pa = cur;         // the matrix of this pass
        bool in_place = false;  // pa is C's own arrays already
        for (int pass = 0; pass < max_passes; ++pass) {
            if (pass > 0) {
                OGL_TRY(grow(M.pass_agg, (size_t)pa.n, st));
                launch_mg_diag(st, pa, M.diag.p, nullptr);
            }
            int32_t nc = 0;
            OGL_TRY(mg_aggregate(st, M, pa, hashed, temp_bytes, pass == 0 ? L.agg.p : M.pass_agg.p, &nc));
            if (nc >= pa.n) break;  // (a pass that does not shrink is dropped and ends the level's passes)
            if (pass == 0)
                OGL_HIP_CHECK(hipMemcpyAsync(L.agg.p, M.cidx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            else
                launch_mg_compose(st, n, M.cidx.p, L.agg.p);
            // (the level's last pass writes the kept level's own arrays; one that may be followed by another, scratch)
            in_place = pass + 1 == max_passes || nc <= min_coarse || nc < 2;
            const MgCsrBufs scratch{M.pass_row_ptrs[pass & 1], M.pass_cols[pass & 1], M.pass_vals[pass & 1]};
            OGL_TRY(mg_galerkin(st, M, pa, nc, temp_bytes, in_place ? kept : scratch, &pa, keep > 0 ? &L : nullptr, L.passes));
            ++L.passes;
            if (in_place) break;
        }
        if (L.passes == 0) break;  // (the first pass did not shrink: the hierarchy ends here)
        // (a later pass was dropped: the kept matrix is the scratch one of the pass before it)
        if (!in_place) OGL_TRY(kept.copy_from(pa, st));
        const int32_t nc = pa.n;
        // ---- the members of every coarse row, ascending (rows[i] = i: k_mg_coarse_index of the first pass) ----
        OGL_TRY(grow(L.agg_ptr, (size_t)nc + 1, st));
        OGL_HIP_CHECK(mg_sort_rows(st, M.temp.p, temp_bytes, L.agg.p, M.sorted.p, M.rows.p, L.agg_rows.p, n));
        launch_mg_member_ptr(st, n, nc, M.sorted.p, L.agg_ptr.p);
        OGL_TRY(grow(C.dbl.b, (size_t)nc + 2, st));
        L.n_coarse = nc;
        C.n = nc;
        C.nnz = pa.nnz;
        cur = C.view<double>();
    }
    M.n_levels = l + 1;
    MgLevel &last = *M.levels[(size_t)l];
    OGL_TRY(grow(last.dbl.r, (size_t)last.n + 2, st));
    OGL_TRY(grow(last.dbl.p, (size_t)last.n + 2, st));
    OGL_TRY(grow(last.part, n_chunks(last.n) + 1, st));
    if (keep > 0) {
        M.kept_for = asking;
        M.kept_left = keep;
    }
    return OGL_OK;
}

// ------------------------------------------------------------------------------------------
// the apply: what the two precisions do differently, then the one cycle
// ------------------------------------------------------------------------------------------
namespace {

// a dot product of the coarsest CG, in the loop's tree: plain in double precision, wide (fp64 products of the casts) in single
void mg_dot(MgRun &run, int32_t n, const double *a, const double *b, double *part)
{
    launch_partials_dot(run.next(), n, a, b, part, run.gate);
}
void mg_dot(MgRun &run, int32_t n, const float *a, const float *b, double *part)
{
    launch_mg_wide_dot(run.next(), n, a, b, part, run.gate);
}

// The first pre-sweep of a visit from x = 0.  Level 0 of the cycle in single precision reads the fp64 residual ends.in, and
// this sweep forms b = fl32(ends.in) on the way.
void mg_first_sweep(MgRun &run, int32_t n, const double *b, const MgWide &ends, const MgOperands<double> &V, double *x)
{
    assert(!ends.in);
    launch_mg_jacobi0<double>(run.next(), n, b, V.inv_d.p, x, run.gate);
}
void mg_first_sweep(MgRun &run, int32_t n, const float *b, const MgWide &ends, const MgOperands<float> &V, float *x)
{
    if (ends.in)
        launch_mg_jacobi0_in(run.next(), n, ends.in, V.inv_d.p, V.b.p, x, run.gate);
    else
        launch_mg_jacobi0<float>(run.next(), n, b, V.inv_d.p, x, run.gate);
}

// a hierarchy of one level in single precision: the coarsest CG's answer goes out as doubles
void mg_widen(MgRun &run, int32_t n, const double *x, const MgWide &ends) { assert(!ends.out); }
void mg_widen(MgRun &run, int32_t n, const float *x, const MgWide &ends)
{
    if (ends.out) launch_mg_widen(run.next(), n, x, ends.out, run.gate);
}

}  // namespace

// Level 0's product in single precision with its epilogue (kernels_mixed.hip): on the fp32 twin of the half storage's
// planes where that is the in-loop layout, else on the fp32 value array beside the device CSR.
void ogl_solver::mg_fine32(MxEpilogue epi, const float *x, const MgEpi &e, MgRun &run)
{
    if (fp32_dev.half)
        launch_mg_fine_sym(run.next(), sym(), fp32_dev.planes.p, epi, x, e);
    else
        launch_mg_fine_csr(run.next(), csr(false), fp32_dev.vals.p, epi, x, e);
}

void ogl_solver::mg_product(const MgLevel &L, const double *x, double *y, MgRun &run)
{
    if (L.own) {
        launch_mg_csr_spmv<double>(run.next(), L.view<double>(), x, y, run.gate);
    } else {
        run.next();  // (spmv_on launches once, on the registry's stream)
        spmv_on(spmv_layout, SPMV_PLAIN, x, nullptr, y, SpmvDots{}, run.gate);
    }
}
void ogl_solver::mg_product(const MgLevel &L, const float *x, float *y, MgRun &run)
{
    if (L.own)
        launch_mg_csr_spmv<float>(run.next(), L.view<float>(), x, y, run.gate);
    else
        mg_fine32(MX_EPI_PLAIN, x, MgEpi{nullptr, nullptr, y, nullptr, run.gate}, run);
}

// A sweep of level 0 on the in-loop layout.  Double precision: the product, then the sweep behind it (two launches).
// Single precision: one launch, the sweep as the product's epilogue -- written as doubles to out64 where that is given
// (the cycle's last sweep).
void ogl_solver::mg_layout_sweep(const MgLevel &L, const double *b, const double *x, double *x_out, double *out64, MgRun &run)
{
    assert(!out64);
    mg_product(L, x, L.dbl.t.p, run);
    launch_mg_sweep_epi(run.next(), L.n, b, L.dbl.t.p, L.dbl.inv_d.p, x, x_out, run.gate);
}
void ogl_solver::mg_layout_sweep(const MgLevel &L, const float *b, const float *x, float *x_out, double *out64, MgRun &run)
{
    const MgEpi e{b, L.flt.inv_d.p, out64 ? nullptr : x_out, out64, run.gate};
    mg_fine32(out64 ? MX_EPI_SWEEP64 : MX_EPI_SWEEP, x, e, run);
}

// What the restriction of level 0 on the in-loop layout reads, left in the level's t: the product A x in double precision,
// the residual b - A x (the product's epilogue) in single precision.
MgRestrictFrom ogl_solver::mg_layout_residual(const MgLevel &L, const double *b, const double *x, MgRun &run)
{
    mg_product(L, x, L.dbl.t.p, run);
    return MG_FROM_AX;
}
MgRestrictFrom ogl_solver::mg_layout_residual(const MgLevel &L, const float *b, const float *x, MgRun &run)
{
    mg_fine32(MX_EPI_RESIDUAL, x, MgEpi{b, L.flt.inv_d.p, L.flt.t.p, nullptr, run.gate}, run);
    return MG_FROM_RES;
}

// The level table of the single-workgroup tail kernel (kernels_mg.hip, k_mg_tail): level `first` and everything below it.
template <class T>
MgTailOf<T> ogl_solver::mg_tail_table(int first, bool continued) const
{
    const MultigridPart &M = precond_data->mg;
    MgTailOf<T> Tl;
    Tl.count = M.n_levels - first;
    Tl.cg_iters = M.cg_iters;
    Tl.coarse_visits = mg_coarse_visits;
    Tl.continued = continued ? 1 : 0;
    Tl.sweeps = mg_sweeps;
    Tl.scale = mg_scale;
    for (int k = 0; k < Tl.count; ++k) {
        const MgLevel &S = *M.levels[(size_t)(first + k)];
        const MgOperands<T> &V = S.ops<T>();
        const MgCsrOf<T> A = mg_matrix<T>(S);
        MgTailLevelOf<T> &D = Tl.lev[k];
        D.n = S.n;
        D.n_coarse = S.n_coarse;
        D.row_ptrs = A.row_ptrs;
        D.cols = A.cols;
        D.vals = A.vals;
        D.inv_d = V.inv_d.p;
        D.agg = S.agg.p;
        D.agg_ptr = S.agg_ptr.p;
        D.agg_rows = S.agg_rows.p;
        D.b = V.b.p;
        D.xa = V.xa.p;
        D.xb = V.xb.p;
        D.t = V.t.p;
        D.r = V.r.p;
        D.p = V.p.p;
        D.part = S.part.p;
    }
    return Tl;
}

// One visit of `level`: x = the cycle's answer to A_level x = b -- from x = 0, or (continued; never level 0 or the coarsest)
// from the answer of the visit before, which x then holds.  x is the level's own xb for every level but 0, so a continued
// visit reads it before the visit's last sweep writes it.  The level's b is not written by its own visits.  T: the operand
// type, the same steps in the same order on either.  Level 0 of the cycle in single precision (`ends` given) reads the
// fp64 residual ends.in -- b = fl32(ends.in) is formed by its first pre-sweep -- and its last post-sweep writes ends.out as
// doubles instead of x.
template <class T>
void ogl_solver::mg_cycle(int level, const T *b, T *x, const MgWide &ends, MgRun &run, bool continued)
{
    const MultigridPart &M = precond_data->mg;
    const MgLevel &L = *M.levels[(size_t)level];
    const MgOperands<T> &V = L.ops<T>();
    const DevScalars *gate = run.gate;
    const int32_t n = L.n;
    if (level >= mg_tail_first) {
        // this level and everything below it: one single-workgroup kernel
        launch_mg_tail<T>(run.next(), mg_tail_table<T>(level, continued), b, x, gate);
        return;
    }
    if (level == M.n_levels - 1) {
        // the coarsest solver: coarseSolverIters iterations of unpreconditioned CG, no criterion; dots in the loop's tree
        MgScalars *sc = M.scal.p;
        const int n_part = (int)n_chunks(n);
        launch_mg_cg_init<T>(run.next(), n, b, ends.in, V.r.p, x, V.p.p, gate);
        for (int it = 0; it < M.cg_iters; ++it) {
            mg_dot(run, n, V.r.p, V.r.p, L.part.p);
            launch_mg_cg_fin(run.next(), L.part.p, n_part, 0, it == 0, sc, gate);
            launch_mg_cg_step1<T>(run.next(), n, V.p.p, V.r.p, sc, gate);
            mg_product(L, V.p.p, V.t.p, run);
            mg_dot(run, n, V.p.p, V.t.p, L.part.p);
            launch_mg_cg_fin(run.next(), L.part.p, n_part, 1, 0, sc, gate);
            launch_mg_cg_step2<T>(run.next(), n, x, V.r.p, V.p.p, V.t.p, sc, gate);
        }
        mg_widen(run, n, x, ends);
        return;
    }
    const MgLevel &C = *M.levels[(size_t)level + 1];
    const MgOperands<T> &Vc = C.ops<T>();
    const MgCsrOf<T> A = L.view<T>();
    const int nu = mg_sweeps;
    const T scale = (T)mg_scale;  // (single precision: fl32 of the keyword's value)
    // level 0 in the caller's numbering: products on the in-loop layout, sweeps behind them (a continued visit never is)
    const bool layout = !L.own;
    // one sweep from `from` into `to`; xc: on t = from + scale xc[agg], the prolongation folded in (CSR levels only)
    const auto sweep = [&](const T *from, const T *xc, T *to, double *to64) {
        if (layout)
            mg_layout_sweep(L, b, from, to, to64, run);
        else
            launch_mg_csr_sweep<T>(run.next(), A, V.inv_d.p, b, from, xc, xc ? L.agg.p : nullptr, scale, to, to64, gate);
    };
    // smootherSweeps pre-sweeps (the first from x = 0: no product; of a continued visit: a full sweep from x), residual and
    // restriction.  x ping-pongs between xa and xb (no sweep writes the vector it reads): the first pre-sweep writes xa, so
    // `cur`, what the last one wrote and the restriction reads, is xa for an odd count and xb for an even one.
    T *cur = V.xa.p;
    const auto other = [&V](const T *v) { return v == V.xa.p ? V.xb.p : V.xa.p; };
    if (continued)
        sweep(x, nullptr, cur, nullptr);
    else
        mg_first_sweep(run, n, b, ends, V, cur);
    for (int k = 1; k < nu; ++k, cur = other(cur)) sweep(cur, nullptr, other(cur), nullptr);
    const MgRestrictFrom from = layout ? mg_layout_residual(L, b, cur, run) : MG_FROM_A;
    launch_mg_restrict<T>(run.next(), C.n, L.agg_ptr.p, L.agg_rows.p, A, b, cur, from, layout ? V.t.p : nullptr, Vc.b.p, gate);
    // the coarse correction lands in the coarse level's xb (its last post-sweep writes there; the coarsest CG too); the
    // visits after the first continue from there with the same C.b
    mg_cycle<T>(level + 1, Vc.b.p, Vc.xb.p, MgWide{}, run, false);
    if (level + 2 < M.n_levels)
        for (int visit = 1; visit < mg_coarse_visits; ++visit) mg_cycle<T>(level + 1, Vc.b.p, Vc.xb.p, MgWide{}, run, true);
    // the scaled correction and smootherSweeps post-sweeps, the last of them into x (level 0: the caller's vector, or
    // ends.out as doubles; below it the level's xb, where the alternation lands whatever the count).  On a CSR level the
    // prolongation is folded into the first post-sweep: t_j = x_j + scale x_c[agg(j)], product and sum rounded once each;
    // on the in-loop layout it keeps a launch of its own.
    if (layout) {
        launch_mg_prolong<T>(run.next(), n, cur, Vc.xb.p, L.agg.p, scale, other(cur), gate);
        cur = other(cur);
    }
    for (int k = 0; k < nu; ++k, cur = other(cur)) {
        const bool end = k == nu - 1;
        sweep(cur, k == 0 && !layout ? Vc.xb.p : nullptr, end ? x : other(cur), end ? ends.out : nullptr);
    }
}
template void ogl_solver::mg_cycle<double>(int, const double *, double *, const MgWide &, MgRun &, bool);
template void ogl_solver::mg_cycle<float>(int, const float *, float *, const MgWide &, MgRun &, bool);

void ogl_solver::apply_multigrid(const double *in, double *out, const DevScalars *gate, double *dot_part)
{
    const MultigridPart &M = precond_data->mg;
    // the tail: the levels of at most mgTailRows rows (this solver's own property, also on a stored hierarchy); never
    // more than the kernel's level table and reduction tree hold
    const double tail_rows = std::min(knob<Knob::mgTailRows>(), (double)MG_TAIL_MAX_ROWS);
    mg_tail_first = M.n_levels;
    while (mg_tail_first > 0 && M.n_levels - mg_tail_first < MG_TAIL_MAX_LEVELS &&
           (double)M.levels[(size_t)mg_tail_first - 1]->n <= tail_rows)
        --mg_tail_first;
    // (single precision: level 0 arrives and leaves in fp64 and takes its products from the in-loop layout's fp32 copy --
    //  it is launched, whatever its size)
    if (mg_single && mg_tail_first < 1) mg_tail_first = 1;
    props["mgTailLevels"] = (double)(M.n_levels - mg_tail_first);
    set_knob<Knob::mgTailRows>(tail_rows);
    MgRun run;
    run.st = reg->stream;
    run.gate = gate;
    // a renumbered device copy: the vectors carried into the caller's order and back, as apply_factor does
    const bool carried = pat.renumbered();
    const double *r = carried ? M.in.p : in;
    double *z = carried ? M.out.p : out;
    if (carried) launch_factor_gather_perm(run.next(), pat.n_rows, d_new_id.p, in, M.in.p, gate);
    if (mg_single) {
        const MgOperands<float> &V0 = M.levels[0]->flt;
        mg_cycle<float>(0, V0.b.p, V0.xb.p, MgWide{r, z}, run, false);
    } else {
        mg_cycle<double>(0, r, z, MgWide{}, run, false);
    }
    if (carried) launch_factor_scatter_perm(run.next(), pat.n_rows, d_new_id.p, z, out, gate);
    props["mgLaunchesPerApply"] = (double)run.launches;  // (without the fused dot of a Krylov turn)
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
        const MgCsr A = s->mg_matrix<double>(L);
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
