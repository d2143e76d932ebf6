// solver_proj.cpp -- the initial guess from the last solutions (keyword guessProjection K).
// A field keeps the steps x_final - x0 of its last K solves.  A solve with k >= 1 of them stored replaces its guess x0 by
// x0 + sum_j alpha_j d_j, alpha minimising |r0 - (A D) alpha|_2 on THIS solve's coefficients, and then runs exactly as
// the same solve called with that guess: everything here happens on d_x before the solve and on the ring after it.
#include <cmath>

#include "solver_internal.hpp"

using namespace ogl;

// Property guessProjection: 0 (off, the default) .. PROJ_MAX stored steps.  The sums of the pre-step go through one
// finaliser launch of their own, which has no all-reduce: with several ranks the solve is refused, not run without the
// projection in silence.
int ogl_solver::proj_requested(int *K)
{
    *K = 0;
    OGL_TRY(check_knob(Knob::guessProjection));
    const double v = knob<Knob::guessProjection>();
    const int n_ranks = reg->comm ? reg->comm->n_ranks : 1;
    if (v != 0.0 && n_ranks > 1)
        return fail(OGL_ERR_UNSUPPORTED, "guessProjection %d runs on one rank: this registry has %d ranks", (int)v, n_ranks);
    *K = (int)v;
    return OGL_OK;
}

// Property guessProjectionCredit: 0 (the default) | 1.  With 1 the criterion's initial residual is counted from the guess
// the caller handed in, S0 / norm_factor, so that relTol credits the projection instead of charging
// for it.  The mixed mode keeps a copy of the criterion of its own, which does not take the credit: refused, not run
// without it in silence.  With K = 0 the keyword has nothing to act on.
int ogl_solver::proj_credit_requested(int K, bool mixed_on, bool *credit)
{
    *credit = false;
    OGL_TRY(check_knob(Knob::guessProjectionCredit));
    const double v = knob<Knob::guessProjectionCredit>();
    if (v == 1.0 && K > 0 && mixed_on)
        return fail(OGL_ERR_UNSUPPORTED,
                    "guessProjectionCredit 1 is not built for mixedPrecision: its outer criterion does not take the credit");
    *credit = v == 1.0 && K > 0;
    return OGL_OK;
}

// Property guessProjectionProducts: 0 (separate, the default: k + 1 launches of the in-loop product) | 1 (onePass)
int ogl_solver::proj_products_requested(bool *one_pass)
{
    *one_pass = knob<Knob::guessProjectionProducts>() == 1.0;
    return check_knob(Knob::guessProjectionProducts);
}

// Called by the solve between the reset of its scalars and its first check: S0 of the pre-step into the criterion's state,
// device to device.  The launch is the same for every solve of the field (rec and the scalar block do not move).
void ogl_solver::proj_credit(hipStream_t st, ogl::DevScalars *s)
{
    if (proj.active && proj.credit && proj.offered >= 1) launch_proj_credit(st, proj.rec(), s);
}

// The ring is cleared by a write of 1 to guessProjectionReset, by a change of K and by a new sparsity pattern; a change of
// coefficients keeps it (W is formed anew in every solve).  With K > 0 the buffers are sized here, once.
int ogl_solver::proj_sync(int K)
{
    if (knob<Knob::guessProjectionReset>() == 1.0) {
        proj.clear();
        set_knob<Knob::guessProjectionReset>(0.0);
    }
    if (K != proj.K || pat_id != proj.pat_id) proj.clear();
    proj.K = K;
    proj.pat_id = pat_id;
    if (K == 0) return OGL_OK;
    hipStream_t st = reg->stream;
    const size_t nc = (size_t)n_chunks(pat.n_rows);
    proj.ld = ((int64_t)pat.n_rows + 3) & ~(int64_t)1;  // (even: a pair of rows is one 16-byte access in every vector)
    OGL_TRY(proj.ring.alloc((size_t)K * (size_t)proj.ld, st));
    OGL_TRY(proj.W.alloc((size_t)K * (size_t)proj.ld, st));
    OGL_TRY(proj.part.alloc((size_t)proj_n_sums(K) * nc + 1, st));
    OGL_TRY(proj.small.alloc(ProjPart::SMALL_LEN, st));
    return OGL_OK;
}

int ogl_solver::proj_pre_step(int K, bool credit, bool one_pass)
{
    proj.active = false;
    proj.credit = credit;
    proj.one_pass = false;
    if (K == 0 && proj.K == 0) return OGL_OK;  // (never asked for: nothing to clear, nothing to publish)
    OGL_TRY(proj_sync(K));
    const int n = pat.n_rows;
    if (K == 0 || n == 0) return OGL_OK;
    hipStream_t st = reg->stream;
    const int k = proj.count;
    const size_t bytes = (size_t)n * sizeof(double);
    proj.offered = k;
    proj.launches = 0;
    proj.active = true;
    proj.timed = k >= 1 && knob<Knob::guessProjectionTimed>() != 0.0;
    auto mark = [&](int i) -> int {
        if (!proj.timed) return OGL_OK;
        if (!proj.ev[i]) OGL_HIP_CHECK(ev_create(&proj.ev[i]));
        OGL_HIP_CHECK(hipEventRecord(proj.ev[i], st));
        return OGL_OK;
    };
    if (k == 0) {  // nothing to project on: x0 kept for the step this solve will store
        OGL_HIP_CHECK(hipMemcpyAsync(proj.W.p, d_x.p, bytes, hipMemcpyDeviceToDevice, st));
        return OGL_OK;
    }
    OGL_TRY(mark(0));
    // r0 = b - A x0 with the prologue's residual product; w_j = A d_j with the in-loop product, oldest first
    // (keyword guessProjectionProducts onePass, whole-matrix half storage only: all k + 1 products in one pass of the planes,
    //  the same bits -- k_proj_products_sym; on every other in-loop layout the keyword is accepted and these launches run)
    proj.one_pass = one_pass && spmv_layout == SpmvLayout::Sym && pat.non_local_nnz == 0;
    if (proj.one_pass) {
        ProjProducts v{};
        for (int j = 0; j < k; ++j) v.in[j] = proj.slot(j);
        v.W = proj.W.p;
        v.ld = (long)proj.ld;
        v.k = k;
        launch_proj_products_sym(st, sym(), d_x.p, d_b.p, d_r.p, v);
        proj.launches += 1;
    } else {
        OGL_TRY(dist_spmv(SPMV_RESIDUAL, d_x.p, d_b.p, d_r.p, SpmvDots{}, nullptr));
        for (int j = 0; j < k; ++j)
            OGL_TRY(dist_spmv(SPMV_PLAIN, proj.slot(j), nullptr, proj.W.p + (size_t)j * (size_t)proj.ld, SpmvDots{}, nullptr));
        proj.launches += 1 + k;
    }
    OGL_TRY(mark(1));
    launch_proj_gram(st, n, d_r.p, proj.W.p, proj.ld, k, proj.part.p, nullptr);
    launch_gmres_fin_h(st, n, nullptr, proj.part.p, proj_n_sums(k), proj.sums(), proj.sums_copy(), false);
    proj.launches += 2;
    OGL_TRY(mark(2));
    launch_proj_solve(st, k, proj.sums(), proj.h(), proj.rec(), nullptr);
    proj.launches += 1;
    OGL_TRY(mark(3));
    // (W has been read: its first vector keeps x0 until the step is stored -- at k = K the slot that step will take still
    //  holds the oldest vector, which this projection uses)
    OGL_HIP_CHECK(hipMemcpyAsync(proj.W.p, d_x.p, bytes, hipMemcpyDeviceToDevice, st));
    // x = x - sum_j h_j d_j, j ascending.  A ring that has wrapped is two runs of slots: the second launch goes on from
    // the x the first one stored, which is the same sequence of roundings per row.
    const int run0 = std::min(k, proj.K - proj.first);
    launch_gmres_block_update(st, n, d_x.p, proj.slot(0), proj.ld, run0, proj.h(), proj.part.p, nullptr, nullptr);
    proj.launches += 1;
    if (run0 < k) {
        launch_gmres_block_update(st, n, d_x.p, proj.ring.p, proj.ld, k - run0, proj.h() + run0, proj.part.p, nullptr, nullptr);
        proj.launches += 1;
    }
    OGL_TRY(mark(4));
    OGL_HIP_CHECK(hipGetLastError());
    return OGL_OK;
}

// After the solve (its stream is idle: krylov_finish has read the final scalars): the kept count, and the step
// x_final - x0 into the ring when the solve succeeded and moved x -- a column was kept or a turn ran.
int ogl_solver::proj_post_step(int rc, const ogl_perf *perf)
{
    if (!proj.active) return rc;
    proj.active = false;
    if (rc != OGL_OK) return rc;  // (the slot is abandoned)
    hipStream_t st = reg->stream;
    double rec[3] = {0.0, 0.0, 0.0};
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    if (proj.offered > 0) OGL_HIP_CHECK(hipMemcpy(rec, proj.rec(), sizeof(rec), hipMemcpyDeviceToHost));
    const int kept = (int)rec[1];
    // (ogl_perf::n_iterations: the checks of GKOCG, GKOGMRES and the mixed mode -- a turn ran from the second on --, the
    //  whole turns of GKOBiCGStab, whose first half-step already moves x)
    const bool turned = perf->n_iterations >= (cfg.solver == OGL_SOLVER_BICGSTAB ? 1 : 2);
    if (kept >= 1 || turned) {
        const int at = proj.count < proj.K ? proj.count : 0;  // (full: the oldest is overwritten and the next one is the oldest)
        launch_proj_delta(st, pat.n_rows, d_x.p, proj.W.p, proj.slot(at), nullptr);
        if (proj.count < proj.K) ++proj.count;
        else proj.first = (proj.first + 1) % proj.K;
        OGL_HIP_CHECK(hipGetLastError());
    }
    props["guessProjectionOffered"] = (double)proj.offered;
    props["guessProjectionKept"] = (double)kept;
    props["guessProjectionStored"] = (double)proj.count;
    props["guessProjectionNormBefore"] = rec[0];
    props["guessProjectionLaunches"] = (double)proj.launches;
    props["guessProjectionOnePassInUse"] = (proj.offered > 0 && proj.one_pass) ? 1.0 : 0.0;
    // (what k_proj_credit decided, from the same three numbers)
    props["guessProjectionCreditInUse"] =
        (proj.credit && proj.offered > 0 && kept >= 1 && rec[0] > 0.0 && std::isfinite(rec[0])) ? 1.0 : 0.0;
    if (proj.timed) {
        static const char *const names[4] = {"guessProjectionProductsMs", "guessProjectionGramMs", "guessProjectionSolveMs",
                                             "guessProjectionUpdateMs"};
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            OGL_HIP_CHECK(hipEventElapsedTime(&ms, proj.ev[i], proj.ev[i + 1]));
            props[names[i]] = (double)ms;
        }
    }
    return OGL_OK;
}

// ogl_solver_set_guess_history / ogl_solver_get_guess_history: the ring in the caller's cell order, oldest first
int ogl_solver::set_guess_history(const double *vectors, int32_t k)
{
    int K = 0;
    OGL_TRY(proj_requested(&K));
    if (k < 0 || k > K) return fail(OGL_ERR_INVALID, "guess history of %d vectors: guessProjection is %d", k, K);
    if (k > 0 && !vectors) return fail(OGL_ERR_INVALID, "NULL argument");
    OGL_TRY(proj_sync(K));
    proj.clear();
    for (int j = 0; j < k; ++j)
        OGL_TRY(upload_rows(proj.ring.p + (size_t)j * (size_t)proj.ld, vectors + (size_t)j * (size_t)pat.n_rows));
    OGL_HIP_CHECK(hipStreamSynchronize(reg->stream));
    proj.count = k;
    return OGL_OK;
}

int ogl_solver::get_guess_history(double *out, int32_t capacity, int32_t *k)
{
    int K = 0;
    OGL_TRY(proj_requested(&K));
    OGL_TRY(proj_sync(K));
    if (proj.count > capacity)
        return fail(OGL_ERR_INVALID, "guess history of %d vectors does not fit a capacity of %d", proj.count, capacity);
    for (int j = 0; j < proj.count; ++j) OGL_TRY(download_rows(out + (size_t)j * (size_t)pat.n_rows, proj.slot(j)));
    *k = proj.count;
    return OGL_OK;
}
