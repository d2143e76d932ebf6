// solver_mixed.cpp -- mixed precision for GKOCG (property mixedPrecision; the contract: DESIGN.md section 7c): the Krylov
// turns run in fp32 on an fp32 copy of the matrix, as the inner solver of an fp64 iterative refinement whose residual,
// criterion, norm factor and x are the double path's own.  The host enqueues and polls as krylov_loop does: batches of
// inner turns with the stop flags looked at one batch late, every kernel past a stop a no-op.
// See solver.hpp, solver_internal.hpp, kernels_mixed.hip.
#include "solver_internal.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

using namespace ogl;

namespace {

const char *solver_name(int kind)
{
    return kind == OGL_SOLVER_CG ? "GKOCG" : kind == OGL_SOLVER_BICGSTAB ? "GKOBiCGStab" : "GKOGMRES";
}

int32_t *word_of(MixedScalars *m, size_t offset) { return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(m) + offset); }

}  // namespace

// The keywords (properties of the same name) and where the mode applies: GKOCG, any number of ranks, preconditioner none or
// BJ with maxBlockSize 1.  Anything else with mixedPrecision set is refused, none silently.
int ogl_solver::mixed_requested(bool *on)
{
    *on = knob<Knob::mixedPrecision>() != 0.0;
    if (!*on) return OGL_OK;
    OGL_TRY(check_knob(Knob::innerRelTol));
    const double inner_max_iter = knob<Knob::innerMaxIter>();
    if (!(inner_max_iter >= 1.0)) return fail(OGL_ERR_INVALID, "innerMaxIter %g below 1", inner_max_iter);
    const PrecondKind kind = precond_kind_of(cfg);
    const bool precond_ok = cfg.preconditioner == OGL_PRECOND_NONE || kind == PrecondKind::Jacobi;
    const int n_ranks = reg->comm ? reg->comm->n_ranks : 1;
    if (cfg.solver != OGL_SOLVER_CG || !precond_ok)
        return fail(OGL_ERR_UNSUPPORTED,
                    "mixedPrecision runs GKOCG with preconditioner none or BJ with maxBlockSize 1: this is "
                    "solver %s, preconditioner %s (maxBlockSize %d), %d rank(s)",
                    solver_name(cfg.solver), cfg.preconditioner == OGL_PRECOND_NONE ? "none" : precond_name(kind),
                    cfg.max_block_size, n_ranks);
    return OGL_OK;
}

// The vectors and scalars of the mode, reset for a solve, and the fp32 copy of the matrix current for this coefficient
// upload: the twin of the half storage's planes when the in-loop SpMV runs there, the value array beside the device
// CSR on every other in-loop layout.
int ogl_solver::mixed_storage(const DevCriterion &crit, double inner_rel_tol, int inner_max_iter)
{
    hipStream_t st = reg->stream;
    const size_t nv = (size_t)pat.n_rows + 4;  // (a trailing pair access of the last odd row stays inside)
    for (DevBuf<float> *b : {&mixed.u, &mixed.r, &mixed.z, &mixed.p, &mixed.q, &mixed.inv_d}) OGL_TRY(b->alloc(nv, st));
    OGL_TRY(mixed.scal.alloc(1, st));
    if (!mixed.h_scal)
        OGL_HIP_CHECK(ledger::pinned_malloc(reinterpret_cast<void **>(&mixed.h_scal), 2 * sizeof(MixedScalars)));
    launch_mixed_reset(st, mixed.scal.p, crit, inner_rel_tol, inner_max_iter);
    const bool half = spmv_layout == SpmvLayout::Sym;
    if (half) refresh_values(SpmvLayout::Sym);
    // (processor interfaces: A32_nl beside it, the halo in fp32 -- nothing but the twin of d_nl_vals is allocated for it)
    OGL_TRY(fp32_dev.ensure(half, pat_id, half ? sym_dev.map.n : d_vals.n, (size_t)pat.non_local_nnz, st));
    if (fp32_dev.epoch != vals_epoch || vals_epoch == 0) {
        fp32_dev.refresh(half ? sym_dev.map.p : nullptr, d_vals.p, d_nl_vals.p,
                         word_of(mixed.scal.p, offsetof(MixedScalars, bad_coef)), st);
        fp32_dev.epoch = vals_epoch;
    }
    props["mixedInnerLayout"] = half ? 2.0 : 0.0;  // (spmvLayout's codes: 2 half storage, 0 the CSR arrays)
    props["mixedHaloBytes"] = peer_halo ? 4.0 : 8.0;  // (bytes per halo value on the wire)
    return OGL_OK;
}

// q = A32 p on this rank's rows.  Several ranks: the neighbours' p32 at their send rows travels while
// the local product runs -- as 4-byte values through the peer mesh, on the sequence and the flags of the double path's
// exchanges; widened to doubles through Comm::exchange on the other rungs -- then the boundary rows continue over their
// non-local entries and the boundary chunks' pi partials are formed again over the finished q.
int ogl_solver::mixed_spmv(const float *x, float *y, double *part, const MixedScalars *gate)
{
    hipStream_t st = reg->stream;
    auto local = [&]() {
        if (fp32_dev.half)
            launch_mixed_spmv_sym(st, sym(), fp32_dev.planes.p, x, y, part, gate);
        else
            launch_mixed_spmv_csr(st, csr(false), fp32_dev.vals.p, x, y, part, gate);
    };
    if (pat.non_local_nnz == 0) {
        local();
        return OGL_OK;
    }
    const MixedHaloOwner own{gate, mixed.scal.p, d_scal.p};
    PeerHalo ph;
    OGL_TRY(halo_begin(x, own, ph));
    local();
    return halo_end(SPMV_PLAIN, ph, fp32_dev.nl_vals.p, y, SpmvDotsOf<float>{x, part, nullptr}, own);
}

// A finaliser of the mode.  Several ranks: its two sums, staged in MixedScalars::sums, are all-reduced between the
// reduction and the logic by the split that ogl_solver::finalize has (split_finaliser, solver_internal.hpp).
int ogl_solver::mixed_fin(int phase, MixedFinArgs &a)
{
    MixedScalars *m = mixed.scal.p;
    double *sums = reinterpret_cast<double *>(reinterpret_cast<char *>(m) + offsetof(MixedScalars, sums));
    return split_finaliser(a, sums, 2, [&] { launch_mixed_fin(reg->stream, phase, m, d_scal.p, a); });
}

// The device row that holds position `position` of fp32_dev's value array (the planes' twin or the CSR values; behind
// them the non-local coefficients, whose row is the boundary row that owns the entry).
int ogl_solver::fp32_bad_row(int64_t position, int64_t *row) const
{
    if (position >= fp32_dev.local_count()) {
        const int64_t e = position - fp32_dev.local_count();
        const size_t i = (size_t)(std::upper_bound(boundary_ptrs.begin(), boundary_ptrs.end(), (int32_t)e) - boundary_ptrs.begin());
        *row = i >= 1 && i - 1 < boundary_rows.size() ? boundary_rows[i - 1] : 0;
        return OGL_OK;
    }
    if (fp32_dev.half) {
        const int64_t per_chunk = (int64_t)sym_dev.nd * CHUNK_ROWS;
        *row = (position / per_chunk) * CHUNK_ROWS + position % CHUNK_ROWS;
        return OGL_OK;
    }
    std::vector<int32_t> rp((size_t)pat.n_rows + 1);
    OGL_HIP_CHECK(hipMemcpy(rp.data(), d_row_ptrs.p, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    *row = (int64_t)(std::upper_bound(rp.begin(), rp.end(), position) - rp.begin()) - 1;
    return OGL_OK;
}

// A coefficient or an inverse diagonal that is finite in fp64 and not in binary32: the solve fails and names the row
// (the caller's numbering).  The copy is marked stale, so that the next call converts -- and reports -- again.  Several
// ranks end such a solve together at its first outer check (bad_global): a rank that owns no such value says so.
int ogl_solver::mixed_overflow(const MixedScalars &m)
{
    if (m.bad_coef == INT_MAX && m.bad_invd == INT_MAX && m.bad_global == 0) return OGL_OK;
    fp32_dev.epoch = 0;
    if (m.bad_coef == INT_MAX && m.bad_invd == INT_MAX)
        return fail(OGL_ERR_INVALID, "mixedPrecision: a value on another rank is finite in double precision and not in single "
                                     "precision (that rank names the row)");
    const bool coef = m.bad_coef != INT_MAX;
    int64_t row = m.bad_invd;
    if (coef) OGL_TRY(fp32_bad_row(m.bad_coef, &row));
    row = std::max<int64_t>(0, std::min<int64_t>(row, (int64_t)pat.n_rows - 1));
    if (pat.renumbered() && (size_t)row < pat.old_of.size()) row = pat.old_of[(size_t)row];
    return fail(OGL_ERR_INVALID, "mixedPrecision: %s of row %lld is finite in double precision and not in single precision",
                coef ? "a coefficient" : "the inverse diagonal", (long long)row);
}

int ogl_solver::run_mixed(ogl_perf *perf)
{
    hipStream_t st = reg->stream;
    const int n = pat.n_rows, nc = (int)n_chunks(n);
    DevScalars *s = d_scal.p;
    const bool is_final = cfg.rel_tol == 0.0;
    // the criterion as configured: every outer check evaluates (frequency 1), the adaptive policy is not consulted
    DevCriterion crit{};
    crit.tolerance = cfg.tolerance;
    crit.rel_tol = cfg.rel_tol;
    crit.min_iter = cfg.min_iter;
    crit.max_iter = cfg.max_iter;
    crit.frequency = 1;
    crit.export_res = cfg.export_res;
    const int inner_max_iter = (int)std::min(knob<Knob::innerMaxIter>(), 2147483647.0);
    OGL_TRY(mixed_storage(crit, knob<Knob::innerRelTol>(), inner_max_iter));
    MixedScalars *m = mixed.scal.p;
    const float *inv_d = nullptr;
    if (precond) {  // inv_d32 = fl32 of the inverse diagonal the double path would use for this solve
        launch_mixed_refresh(st, n, nullptr, precond, mixed.inv_d.p, word_of(m, offsetof(MixedScalars, bad_invd)));
        inv_d = mixed.inv_d.p;
    }
    float *z = inv_d ? mixed.z.p : mixed.r.p;  // without a preconditioner z is the residual itself
    // (sized by what the keywords allow, as the double path's block: the same one solve after solve)
    OGL_TRY(d_history.alloc((size_t)std::max(std::max(crit.max_iter, crit.min_iter) + 2,
                                             crit.max_iter + std::max(1, cfg.norm_eval_limit) + 1) + 4, st));
    if (cfg.export_res) OGL_HIP_CHECK(hipMemsetAsync(d_history.p, 0, d_history.n * sizeof(double), st));
    for (int i = 0; i < 2; ++i)
        if (!chk_ev[i]) OGL_HIP_CHECK(ev_create(&chk_ev[i]));

    // O0: the double path's prologue -- norm factor, r = b - A x on the in-loop layout, the partials of sum |r|
    const double t_start = now_ms();
    launch_reset_scalars(st, s, crit);
    double n_global = (double)n;
    if (reg->comm->multi()) {  // the global row count, as krylov_plan has it
        const double mine[2] = {(double)n, 0.0};
        double got[2] = {0.0, 0.0};
        OGL_HIP_CHECK(hipMemcpyAsync(sums_ptr(s), mine, sizeof(mine), hipMemcpyHostToDevice, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_TRY(reg->allreduce(sums_ptr(s), 2));
        OGL_HIP_CHECK(hipMemcpyAsync(got, sums_ptr(s), sizeof(got), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        n_global = got[0];
    }
    launch_partials_sum(st, n, d_x.p, d_part0.p);
    FinArgs fa{};
    fa.part[0] = d_part0.p;
    fa.n_part = nc;
    fa.n_sums = 1;
    fa.n_local = (double)n;
    fa.n_global = n_global;
    OGL_TRY(finalize(FIN_MEAN, fa));
    launch_fill_xbar(st, n, d_w.p, s);
    OGL_TRY(dist_spmv(SPMV_PLAIN, d_w.p, nullptr, d_q.p, SpmvDots{}, nullptr));
    OGL_TRY(dist_spmv(SPMV_RESIDUAL, d_x.p, d_b.p, d_r.p, SpmvDots{}, nullptr));
    launch_partials_normfactor(st, n, d_b.p, d_q.p, d_r.p, d_part0.p);
    fa = FinArgs{};
    fa.part[0] = d_part0.p;
    fa.n_part = nc;
    fa.n_sums = 1;
    OGL_TRY(finalize(FIN_NORMFACTOR, fa));
    launch_partials_norm1(st, n, d_r.p, d_part2.p);

    auto poll_record = [&](int slot) -> int {
        OGL_HIP_CHECK(hipMemcpyAsync(&mixed.h_scal[slot], m, sizeof(MixedScalars), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipEventRecord(poll_ev[slot], st));
        return OGL_OK;
    };
    // one inner turn, five launches: step 1 | SpMV (pi partials) | a | steps 4, 5 (rho, tau partials) | rho, tau, the gate
    // (several ranks: + the halo's put and finish; every rank enqueues the same launches and calls the same collectives
    //  whatever its row count -- a finaliser runs on a rank without rows too)
    MixedFinArgs f_head{}, f_pi{}, f_rho{};
    f_head.part[0] = d_part2.p;
    f_head.history = d_history.p;
    f_pi.part[0] = d_part2.p;
    f_rho.part[0] = d_part0.p;
    f_rho.part[1] = d_part1.p;
    f_head.n_part = f_pi.n_part = f_rho.n_part = nc;
    auto enqueue_turns = [&](int count) -> int {
        for (int i = 0; i < count; ++i) {
            launch_mixed_step1(st, n, mixed.p.p, z, m);
            OGL_TRY(mixed_spmv(mixed.p.p, mixed.q.p, d_part2.p, m));
            OGL_TRY(mixed_fin(MIXED_FIN_PI, f_pi));
            launch_mixed_step2(st, n, mixed.u.p, mixed.r.p, mixed.p.p, mixed.q.p, inv_d, mixed.z.p, d_part0.p, d_part1.p, m);
            OGL_TRY(mixed_fin(MIXED_FIN_RHO, f_rho));
        }
        return OGL_OK;
    };
    const int batch = 16;
    int turns = 0, enqueued = 0;  // inner turns so far (the device's total_turns); turns put into the stream
    MixedScalars fin{};
    for (int k = 0;; ++k) {
        // O1, O2 (one launch), O3 + the start of the inner solve
        if (k == 0) OGL_HIP_CHECK(hipEventRecord(chk_ev[0], st));
        OGL_TRY(mixed_fin(MIXED_FIN_HEAD, f_head));
        if (k == 0) OGL_HIP_CHECK(hipEventRecord(chk_ev[1], st));
        launch_mixed_start(st, n, d_r.p, inv_d, mixed.r.p, z, mixed.u.p, d_part0.p, d_part1.p, m);
        OGL_TRY(mixed_fin(MIXED_FIN_START, f_rho));
        // O4: the device's budget of this step is min(innerMaxIter, maxIter - T); the host knows T exactly, so it never
        // enqueues past it, and it looks at the flags of batch j only after batch j + 1 is in the queue
        const int cap = std::max(0, std::min(inner_max_iter, crit.max_iter - turns));
        int enq = 0;
        auto next_batch = [&]() -> int {
            const int count = std::min(batch, cap - enq);
            OGL_TRY(enqueue_turns(count));
            enq += count;
            enqueued += count;
            return OGL_OK;
        };
        OGL_TRY(next_batch());
        OGL_TRY(poll_record(0));
        MixedScalars seen{};
        for (int j = 0;; ++j) {
            const bool more = enq < cap;
            if (more) {
                OGL_TRY(next_batch());
                OGL_TRY(poll_record((j + 1) & 1));
            }
            OGL_HIP_CHECK(hipEventSynchronize(poll_ev[j & 1]));
            seen = mixed.h_scal[j & 1];
            if (seen.outer_stop || seen.inner_stop) break;
            if (!more) return fail(OGL_ERR_STATE, "mixedPrecision: the inner solve did not stop within its budget");
        }
        if (seen.outer_stop) {
            fin = seen;
            break;
        }
        turns += seen.inner_turns;
        // O5, O6: x += S u, r = b - A x with the prologue's kernel, the partials of sum |r| for the next check
        launch_mixed_add(st, n, d_x.p, mixed.u.p, m);
        OGL_TRY(dist_spmv(SPMV_RESIDUAL, d_x.p, d_b.p, d_r.p, SpmvDots{}, s));
        launch_partials_norm1(st, n, d_r.p, d_part2.p);
    }
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    if (fin.comm_error)
        return fail(OGL_ERR_COMM, "mixedPrecision: peer all-reduce or halo exchange timed out: a rank did not take part "
                                  "(outer step %d, inner turn %d)", fin.outer_steps, fin.inner_turns);
    if (fin.stop_reason == MIXED_STOP_INVALID) OGL_TRY(mixed_overflow(fin));
    const double t_solve = now_ms() - t_start;
    // where the turns waited: the inner solve's exchanges and sums (MixedScalars) and the double path's of O0 and O6
    DevScalars outer{};
    if (reg->comm->multi()) OGL_HIP_CHECK(hipMemcpy(&outer, s, sizeof(outer), hipMemcpyDeviceToHost));
    props["haloWaits"] = (double)fin.halo_waits + (double)outer.halo_waits;
    props["haloWaitUs"] = ((double)fin.halo_wait_ticks + (double)outer.halo_wait_ticks) / 100.0;
    props["allreduceWaits"] = (double)fin.reduce_waits + (double)outer.reduce_waits;
    props["allreduceWaitUs"] = ((double)fin.reduce_wait_ticks + (double)outer.reduce_wait_ticks) / 100.0;
    props["peerSafeWaitInUse"] = (pat.non_local_nnz > 0 && peer_halo && peer_safe_wait()) ? 1.0 : 0.0;
    props["peerSharedDevice"] = reg->peer_shared_device ? 1.0 : 0.0;
    history.clear();
    if (cfg.export_res) {  // entry j: the j-th evaluated check
        history.resize((size_t)fin.n_evals);
        OGL_HIP_CHECK(hipMemcpy(history.data(), d_history.p, history.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    float chk_ms = 0.f;
    OGL_HIP_CHECK(hipEventElapsedTime(&chk_ms, chk_ev[0], chk_ev[1]));
    props["mixedPrecisionInUse"] = 1.0;
    props["mixedOuterSteps"] = (double)fin.outer_steps;
    props["mixedInnerTurns"] = (double)fin.total_turns;
    props["mixedStopReason"] = (double)fin.stop_reason;
    props["turnsEnqueued"] = (double)enqueued;
    perf->initial_residual = fin.init_res;
    perf->final_residual = fin.res;
    perf->n_iterations = fin.total_turns + 1;  // (maxIter keeps its meaning as a cap on turns)
    perf->n_norm_evals = fin.n_evals;
    perf->norm_factor = fin.norm_factor;
    perf->t_solve_ms = t_solve;
    perf->spmv_avg_ms = 0;
    perf->spmv_launches = 0;
    is_final ? set_knob<Knob::prevSolveIters_final>(perf->n_iterations) : set_knob<Knob::prevSolveIters>(perf->n_iterations);
    const double res_norm_time = std::max(1e-3, (double)chk_ms * 1e3);
    perf->t_res_norm_us = res_norm_time;
    perf->n_global_rows = n_global;
    set_knob<Knob::_prev_solve>(std::floor(t_solve * 1e3 / std::max(perf->n_iterations, 1) / res_norm_time));
    return OGL_OK;
}

// y = A32 x through the inner SpMV of the layout in use, both vectors in the caller's order.  Several ranks: the
// distributed product, collective -- every rank calls it.
int ogl_solver::spmv_f32(const float *x, float *y)
{
    hipStream_t st = reg->stream;
    const int n = pat.n_rows;
    OGL_TRY(mixed_storage(DevCriterion{}, 1e-4, 1));
    const size_t bytes = (size_t)n * sizeof(float);
    if (pat.renumbered()) {
        OGL_TRY(mixed.io.alloc((size_t)n + 4, st));
        OGL_TRY(reg->stager.h2d(mixed.io.p, x, bytes, st));
        launch_mixed_permute(st, n, d_new_id.p, mixed.io.p, mixed.p.p, /*gather=*/false);
    } else {
        OGL_TRY(reg->stager.h2d(mixed.p.p, x, bytes, st));
    }
    OGL_TRY(mixed_spmv(mixed.p.p, mixed.q.p, nullptr, nullptr));
    // property mixedTimedSpmvs > 0 (measurements only): that many inner SpMVs with the pi partials, as a turn runs them,
    // timed with HIP events -> mixedSpmvUs
    if (const int timed = (int)knob<Knob::mixedTimedSpmvs>(); timed > 0) {
        EventPair ev;
        OGL_HIP_CHECK(ev_create(&ev[0]));
        OGL_HIP_CHECK(ev_create(&ev[1]));
        OGL_HIP_CHECK(hipMemcpyAsync(mixed.r.p, mixed.p.p, bytes, hipMemcpyDeviceToDevice, st));
        OGL_TRY(mixed_spmv(mixed.r.p, mixed.z.p, d_part2.p, nullptr));  // warm-up
        OGL_HIP_CHECK(hipEventRecord(ev[0], st));
        for (int i = 0; i < timed; ++i)  // (alternating inputs: no launch reads what the last one wrote)
            OGL_TRY(mixed_spmv((i & 1) ? mixed.r.p : mixed.p.p, mixed.z.p, d_part2.p, nullptr));
        OGL_HIP_CHECK(hipEventRecord(ev[1], st));
        OGL_HIP_CHECK(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        OGL_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        props["mixedSpmvUs"] = 1e3 * (double)ms / timed;
    }
    MixedScalars got;
    OGL_HIP_CHECK(hipMemcpyAsync(&mixed.h_scal[0], mixed.scal.p, sizeof(MixedScalars), hipMemcpyDeviceToHost, st));
    if (pat.renumbered()) {
        launch_mixed_permute(st, n, d_new_id.p, mixed.q.p, mixed.io.p, /*gather=*/true);
        OGL_TRY(reg->stager.d2h(y, mixed.io.p, bytes, st));
    } else {
        OGL_TRY(reg->stager.d2h(y, mixed.q.p, bytes, st));
    }
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    got = mixed.h_scal[0];
    if (got.comm_error)
        return fail(OGL_ERR_COMM, "spmv_f32: halo exchange timed out: a neighbour's values did not arrive");
    return mixed_overflow(got);
}
