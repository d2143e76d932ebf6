// solver_precond.cpp -- the preconditioners other than Multigrid (solver_mg.cpp), Preconditioner.H:47-258,353-431:
//   * generate_preconditioner: the dispatch on the kind with the common tail (serial, numbering record), and one
//     generator per family -- generate_jacobi, generate_block_jacobi, generate_isai, generate_factor, generate_chebyshev --
//     each laid out as
//     "pattern-only part if the object does not hold it for this pattern, then the values"
//   * apply_preconditioner (every kind) with apply_factor and apply_chebyshev, and the breakdown checks
//   * prepare_apply: the applying solver's scratch vectors and launch schedule
//   * init_preconditioner: validate -> caching rule -> generate or adopt -> prepare_apply -> timed applies
//   * precond_current
// The kinds, the parts of PrecondData and the numbering rules: solver.hpp.  The pattern-only host work: host_matrix.hpp
// (find_jacobi_blocks, build_isai_structure, build_factor_structure).
#include "solver_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ogl;

namespace {

// a host array as a device buffer of at least one element
template <class T>
int upload(DevBuf<T> &d, const std::vector<T> &h, size_t pad, Stager &stager, hipStream_t st)
{
    OGL_TRY(d.alloc(std::max<size_t>(1, h.size() + pad), st));
    if (!h.empty()) OGL_TRY(stager.h2d(d.p, h.data(), h.size() * sizeof(T), st));
    return OGL_OK;
}

}  // namespace

int ogl_solver::generate_preconditioner(PrecondData &P)
{
    // structures of a renumbered device copy (block-Jacobi blocks, ISAI(spd)'s triangle) in the CALLER's numbering:
    // the reference's operator (property precondCallerNumbering 0 = the backend's numbering, for A/B)
    const bool caller_numbering = knob<Knob::precondCallerNumbering>() != 0.0;
    if (P.struct_caller_numbering != caller_numbering) P.struct_pat_id = 0;  // (the switch was flipped: rebuild)
    P.struct_caller_numbering = caller_numbering;
    const PrecondKind kind = precond_kind_of(cfg);
    switch (kind) {
    case PrecondKind::Jacobi: OGL_TRY(generate_jacobi(P)); break;
    case PrecondKind::BlockJacobi: OGL_TRY(generate_block_jacobi(P, pat.renumbered() && caller_numbering)); break;
    case PrecondKind::Isai:
    case PrecondKind::Gisai: OGL_TRY(generate_isai(P, caller_numbering)); break;
    case PrecondKind::Ic:
    case PrecondKind::Ilu:
    case PrecondKind::Irilu: OGL_TRY(generate_factor(P)); break;
    // Pgm + Multigrid (Preconditioner.H:259-341) on the local matrix in the caller's numbering; the aggregates depend on
    // the values, so nothing of it is pattern-only (solver_mg.cpp)
    case PrecondKind::Multigrid: OGL_TRY(generate_multigrid(P)); break;
    case PrecondKind::Chebyshev: OGL_TRY(generate_chebyshev(P)); break;
    case PrecondKind::None: return fail(OGL_ERR_UNSUPPORTED, "preconditioner kind %d is not built", cfg.preconditioner);
    }
    P.kind = kind;
    P.stride = precond_stride(kind);
    P.n_rows = (size_t)pat.n_rows;
    static uint64_t serials = 0;
    P.serial = ++serials;
    P.gen_pat_id = pat_id;
    P.gen_device_numbering = pat.renumbered() && !P.keeps_caller_order();  // (see PrecondData::foreign_to)
    return OGL_OK;
}

// scalar Jacobi: 1 / diag
int ogl_solver::generate_jacobi(PrecondData &P) { return generate_inv_diag(P.bj.values); }

int ogl_solver::generate_inv_diag(DevBuf<double> &inv_diag)
{
    hipStream_t st = reg->stream;
    const size_t n = (size_t)pat.n_rows;
    OGL_TRY(inv_diag.alloc(n + 2, st));
    // the diagonal sits contiguous in the staged source of the last coefficient update when the device rows are the
    // caller's cells and no same-rank interface adds entries: 1/d from there (216^3: 124 -> ~25 us per generation,
    // 562 MB of CSR values not touched); otherwise from the CSR values through the diagonal positions -- same bits
    const bool from_source = source_diag_valid && d_new_id.n == 0 && pat.local_iface_nnz == 0 &&
                             d_source.n >= (size_t)pat.diag_start() + (size_t)n && knob<Knob::jacobiFromSource>() != 0.0;
    props["jacobiFromSourceInUse"] = from_source ? 1.0 : 0.0;
    if (from_source)
        launch_jacobi_generate_diag(st, (int32_t)n, d_source.p + pat.diag_start(), inv_diag.p);
    else
        launch_jacobi_generate_pos(st, csr(), d_diag_pos.p, inv_diag.p);
    return OGL_OK;
}

// Chebyshev: w = 1 / d as scalar Jacobi forms it, the Gershgorin bound of D^-1 A over the device CSR
// copy unless chebyshevLambdaMax replaces it, and the table of the recurrence -- three launches, no device-to-host read.
// The keywords were validated in init_preconditioner (check_chebyshev_keywords).
int ogl_solver::generate_chebyshev(PrecondData &P)
{
    hipStream_t st = reg->stream;
    ChebPart &C = P.cheb;
    OGL_TRY(generate_inv_diag(C.w));
    OGL_TRY(C.table.alloc(1, st));
    const double forced = keyword<ChebKeyword::chebyshevLambdaMax>();
    OGL_HIP_CHECK(hipMemsetAsync(C.table.p, 0, sizeof(ChebTable), st));
    if (!(forced > 0.0)) launch_cheb_bound(st, csr(), d_diag_pos.p, C.table.p);
    C.degree = (int)keyword<ChebKeyword::chebyshevDegree>();
    launch_cheb_coeffs(st, pat.n_rows, C.degree, keyword<ChebKeyword::chebyshevEigRatio>(), forced, C.table.p);
    return OGL_OK;
}

int ogl_solver::check_chebyshev_keywords()
{
    OGL_TRY(check_entry(knob_entry(ChebKeyword::chebyshevDegree)));
    OGL_TRY(check_entry(knob_entry(ChebKeyword::chebyshevEigRatio)));
    const double forced = keyword<ChebKeyword::chebyshevLambdaMax>();
    if (!(forced >= 0.0) || !std::isfinite(forced))
        return fail(OGL_ERR_INVALID, "chebyshevLambdaMax %g is not 0 (the bound is computed) or a finite number > 0", forced);
    return OGL_OK;
}

// z^1 = (r w) c0, then `degree` steps z^(k+1) = (z^k + a_k (z^k - z^(k-1))) + b_k (w (r - A_loc z^k)), z^(k+1) written over
// z^(k-1): the iterates alternate between `out` and one scratch vector, assigned so that the last one lands in `out`.
// Fused (this solver's in-loop layout is the whole-matrix half storage): one launch per step; else the residual product
// of the layout in use, local part only, into a second scratch vector and the elementwise step behind it.
void ogl_solver::apply_chebyshev(const double *in, double *out, const DevScalars *gate, double *dot_part)
{
    hipStream_t st = reg->stream;
    const ChebPart &C = precond_data->cheb;
    const int32_t n = pat.n_rows;
    const int degree = C.degree;
    double *odd = degree % 2 == 0 ? out : d_cheb_tmp[0].p, *even = degree % 2 == 0 ? d_cheb_tmp[0].p : out;  // z^1, z^3, .. | z^2, ..
    launch_cheb_first(st, n, in, C.w.p, C.table.p, odd, gate);
    for (int k = 1; k <= degree; ++k) {
        const double *z = k % 2 ? odd : even;
        double *z_io = k % 2 ? even : odd;
        double *part = k == degree ? dot_part : nullptr;
        if (cheb_fused) {
            launch_cheb_step_sym(st, sym(), k, in, C.w.p, C.table.p, z, z_io, part, gate);
        } else {
            spmv_on(spmv_layout, SPMV_RESIDUAL, z, in, d_cheb_tmp[1].p, SpmvDots{}, gate);
            launch_cheb_step(st, n, k, d_cheb_tmp[1].p, C.w.p, C.table.p, z, z_io, in, part, gate);
        }
    }
}

// Jacobi factory with max_block_size = maxBlockSize, skip_sorting (Preconditioner.H:100-104)
int ogl_solver::generate_block_jacobi(PrecondData &P, bool through_perm)
{
    hipStream_t st = reg->stream;
    BlockJacobiPart &B = P.bj;
    const int32_t k = cfg.max_block_size;
    if (!P.has_structure(pat_id, PrecondKind::BlockJacobi, k)) {
        P.struct_pat_id = 0;
        std::vector<int32_t> ptrs, row_block;
        OGL_TRY(download_local_pattern(pat));
        find_jacobi_blocks(pat, k, ptrs, row_block, P.struct_caller_numbering);
        B.n_blocks = (int32_t)ptrs.size() - 1;
        B.uniform_blocks = true;
        for (int32_t b = 0; b + 1 < B.n_blocks; ++b)
            B.uniform_blocks = B.uniform_blocks && ptrs[(size_t)b + 1] - ptrs[(size_t)b] == k;
        if (B.n_blocks > 0) B.uniform_blocks = B.uniform_blocks && ptrs[(size_t)B.n_blocks - 1] == (B.n_blocks - 1) * k;
        OGL_TRY(B.block_ptrs.alloc(ptrs.size(), st));
        OGL_TRY(reg->stager.h2d(B.block_ptrs.p, ptrs.data(), ptrs.size() * sizeof(int32_t), st));
        OGL_TRY(upload(B.row_block, row_block, 0, reg->stager, st));
        P.set_structure(pat_id, PrecondKind::BlockJacobi, k);
    }
    // (not part of the structure: scalar Jacobi may have resized the buffer it shares since)
    OGL_TRY(B.values.alloc(std::max<size_t>(1, (size_t)B.n_blocks * (size_t)k * (size_t)k), st));
    // blocks of the caller's numbering are reached through the permutation.  Staged apply (default): they stay
    // block-major in the caller's order, the vectors are carried there and back by two gather kernels -- one scattered
    // access per row instead of one per block member (128^3 shuffled, BJ(4): 316 us per turn with the direct apply on
    // block rows stored by device row)
    B.through_perm = through_perm;
    B.perm_pat_id = through_perm ? pat_id : 0;
    B.by_device_row = through_perm && knob<Knob::bjStagedApply>() == 0.0;
    const DevBlockJacobi J = B.view(pat.n_rows, k, through_perm ? d_new_id.p : nullptr, through_perm ? d_old_of.p : nullptr);
    launch_bj_generate(st, csr(), J, knob<Knob::bjGroupLanes>() != 0.0);
    return OGL_OK;
}

// Isai<spd|general> with sparsity_power and skip_sorting (Preconditioner.H:225-258).  Pattern of W on the host (tril(A)
// for spd, A for general), its transpose + map for spd (build_isai_structure); values on the device, one dense solve
// per row.
int ogl_solver::generate_isai(PrecondData &P, bool caller_numbering)
{
    hipStream_t st = reg->stream;
    IsaiPart &I = P.isai;
    const bool spd = cfg.preconditioner == OGL_PRECOND_ISAI;
    const PrecondKind kind = spd ? PrecondKind::Isai : PrecondKind::Gisai;
    const int32_t N = pat.n_rows;
    if (!P.has_structure(pat_id, kind, cfg.sparsity_power)) {
        P.struct_pat_id = 0;
        IsaiStructure S;
        ogl_label wide = -1;
        OGL_TRY(download_local_pattern(pat));
        // scratch for the dense systems of the huge rows: batches of rows within a budget (property, bytes)
        const int64_t budget = (int64_t)(knob<Knob::isaiScratchBytes>() / sizeof(double));
        if (!build_isai_structure(pat, spd, cfg.sparsity_power, caller_numbering,
                                  IsaiRowClasses{ISAI_THREAD_ROW, MAX_ISAI_ROW, MAX_ISAI_HUGE_ROW}, budget, S, wide))
            return fail(OGL_ERR_UNSUPPORTED,
                        "preconditioner %s, sparsityPower %d: row %d of the approximate inverse has more than %d "
                        "pattern entries (lower sparsityPower)", precond_name(kind), cfg.sparsity_power, wide,
                        MAX_ISAI_HUGE_ROW);
        I.huge_batches = S.huge_batches;
        I.n_wide_rows = (int32_t)S.wide_rows.size();
        I.n_huge_rows = (int32_t)S.huge_rows.size();
        OGL_TRY(upload(I.wide_rows, S.wide_rows, 0, reg->stager, st));
        OGL_TRY(upload(I.huge_rows, S.huge_rows, 0, reg->stager, st));
        OGL_TRY(upload(I.huge_off, S.huge_off, 0, reg->stager, st));
        I.huge_scratch_len = S.scratch_len;
        I.huge_scratch.release();
        props["isaiWideRows"] = (double)S.wide_rows.size();
        props["isaiHugeRows"] = (double)S.huge_rows.size();
        // (property isaiSortRows 0: W / W^T on the compressed layout only where their own row order qualifies, A/B)
        const bool sort_w = knob<Knob::isaiSortRows>() != 0.0;
        auto compress = [&](SellDev &d, const std::vector<int32_t> &rp, const std::vector<int32_t> &c) -> int {
            OGL_TRY(d.build(N, rp.data(), c.data(), reg->stager, st));
            if (!d.ready && sort_w) OGL_TRY(d.build(N, rp.data(), c.data(), reg->stager, st, true));
            return OGL_OK;
        };
        const size_t wn = S.cols.size();
        OGL_TRY(upload(I.w_row_ptrs, S.row_ptrs, 0, reg->stager, st));
        OGL_TRY(upload(I.w_cols, S.cols, NNZ_PAD, reg->stager, st));
        OGL_TRY(I.w_vals.alloc(wn + NNZ_PAD, st));
        if (spd) {
            OGL_TRY(upload(I.wt_row_ptrs, S.t_row_ptrs, 0, reg->stager, st));
            OGL_TRY(upload(I.wt_cols, S.t_cols, NNZ_PAD, reg->stager, st));
            OGL_TRY(upload(I.wt_map, S.t_map, NNZ_PAD, reg->stager, st));
            OGL_TRY(I.wt_vals.alloc(wn + NNZ_PAD, st));
            if (cfg.compress_indices) OGL_TRY(compress(I.wt_sell, S.t_row_ptrs, S.t_cols));
        }
        if (!spd || !cfg.compress_indices) I.wt_sell.ready = false;
        I.w_sell.ready = false;
        if (cfg.compress_indices) OGL_TRY(compress(I.w_sell, S.row_ptrs, S.cols));
        props["isaiWSorted"] = I.w_sell.sorted ? 1.0 : 0.0;
        props["isaiWtSorted"] = I.wt_sell.sorted ? 1.0 : 0.0;
        I.w_nnz = (int32_t)wn;
        I.w_max_row = S.max_row;
        props["isaiWCompressed"] = I.w_sell.ready ? 1.0 : 0.0;
        props["isaiWtCompressed"] = I.wt_sell.ready ? 1.0 : 0.0;
        P.set_structure(pat_id, kind, cfg.sparsity_power);
    }
    launch_isai_generate(st, csr(), spd ? 1 : 0, I.w_row_ptrs.p, I.w_cols.p, I.w_vals.p, I.w_max_row, I.wide_rows.p,
                         I.n_wide_rows, knob<Knob::isaiGroupLanes>() != 0.0);
    // the dense systems of the huge rows live in a scratch of up to isaiScratchBytes that only this generation
    // needs: allocated here, released below (a field's own preconditioner plus the registry-wide cached one would
    // otherwise sit on 2 GiB each for the whole run)
    if (I.n_huge_rows > 0) OGL_TRY(I.huge_scratch.alloc((size_t)I.huge_scratch_len, st));
    for (size_t bt = 0; bt + 1 < I.huge_batches.size(); ++bt)  // (stream order: a batch reuses the scratch)
        launch_isai_generate_huge(st, csr(), spd ? 1 : 0, I.w_row_ptrs.p, I.w_cols.p, I.w_vals.p, I.huge_rows.p,
                                  I.huge_off.p, I.huge_batches[bt], I.huge_batches[bt + 1] - I.huge_batches[bt],
                                  I.huge_scratch.p);
    if (I.n_huge_rows > 0 && knob<Knob::isaiKeepScratch>() == 0.0) {
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        I.huge_scratch.release();
    }
    if (spd) launch_gather_coeffs(st, I.w_nnz, I.wt_map.p, I.w_vals.p, I.wt_vals.p);
    I.w_sell.refresh(I.w_vals.p, st);
    if (spd) I.wt_sell.refresh(I.wt_vals.p, st);
    return OGL_OK;
}

// factorization::Ic / Ilu (Preconditioner.H:106-126,147-178) on the local matrix in the caller's numbering.
// Pattern-only part on the host (FactorStructure), values gathered and factored on the device level by level.
int ogl_solver::generate_factor(PrecondData &P)
{
    hipStream_t st = reg->stream;
    FactorPart &F = P.fac;
    const bool ic = cfg.preconditioner == OGL_PRECOND_IC;
    const PrecondKind skind = ic ? PrecondKind::Ic : PrecondKind::Ilu;  // (ILU and IRILU share the factor)
    // keywords of the generating solve (validated in init_preconditioner): recorded in the object, which is applied the
    // way it was generated
    const bool want_isai = knob<Knob::triangularSolves>() == 1.0 && cfg.preconditioner != OGL_PRECOND_IRILU;
    const int sweeps = (int)knob<Knob::factorSweeps>();
    const int power = cfg.sparsity_power;
    const bool have = P.has_structure(pat_id, skind, 0);
    const bool need_w = want_isai && !(F.w_pat_id == pat_id && F.w_power == power && F.w_ic == ic);
    const bool need_gs = sweeps > 0 && !ic && F.gs_pat_id != pat_id;
    if (!have || need_w || need_gs) {
        OGL_TRY(download_local_pattern(pat));
        FactorStructure S;
        ogl_label bad = -1;
        if (!build_factor_structure(pat, ic, S, bad))
            return fail(OGL_ERR_INVALID, "preconditioner %s: row %d has no diagonal entry", precond_name(precond_kind_of(cfg)),
                        bad);
        // (first what can refuse: the object stays what it was)
        std::vector<int32_t> w_rp, w_c, wt_rp, wt_c, wt_m;
        if (need_w && !factor_isai_pattern(S, power, FACTOR_ISAI_MAX_ROW, w_rp, w_c, wt_rp, wt_c, wt_m, bad))
            return fail(OGL_ERR_UNSUPPORTED,
                        "preconditioner %s, triangularSolves isai, sparsityPower %d: row %d of the approximate inverse has "
                        "more than %d pattern entries (lower sparsityPower)", precond_name(skind), power, bad,
                        FACTOR_ISAI_MAX_ROW);
        if (!have) {
            P.struct_pat_id = 0;
            const std::pair<DevBuf<int32_t> *, const std::vector<int32_t> *> arrays[] = {
                {&F.row_ptrs, &S.row_ptrs}, {&F.cols, &S.cols},         {&F.diag, &S.diag},         {&F.map_ptr, &S.map_ptr},
                {&F.map, &S.map},           {&F.upd_ptr, &S.upd_ptr},   {&F.upd_a, &S.upd_a},       {&F.upd_b, &S.upd_b},
                {&F.t_row_ptrs, &S.t_row_ptrs}, {&F.t_cols, &S.t_cols}, {&F.t_map, &S.t_map},       {&F.fwd_ptr, &S.fwd_ptr},
                {&F.fwd_rows, &S.fwd_rows}, {&F.bwd_ptr, &S.bwd_ptr},   {&F.bwd_rows, &S.bwd_rows}};
            for (const auto &a : arrays) OGL_TRY(upload(*a.first, *a.second, 0, reg->stager, st));
            F.n_rows = pat.n_rows;
            F.ic = ic;
            F.nnz = (int32_t)S.cols.size();
            OGL_TRY(F.vals.alloc(std::max<size_t>(1, S.cols.size()), st));
            if (ic) OGL_TRY(F.t_vals.alloc(std::max<size_t>(1, S.cols.size()), st));
            else F.t_vals.release();
            OGL_TRY(F.breakdown.alloc(1, st));
            F.fwd_ptr_h = S.fwd_ptr;
            F.bwd_ptr_h = S.bwd_ptr;
            props["iluUpdates"] = (double)S.upd_a.size();
            P.set_structure(pat_id, skind, 0);
        }
        if (need_gs) {
            F.gs_pat_id = 0;
            std::vector<int32_t> gp, ga, gb;
            build_factor_gather_lists(S, gp, ga, gb);
            OGL_TRY(upload(F.gs_ptr, gp, 0, reg->stager, st));
            OGL_TRY(upload(F.gs_a, ga, 0, reg->stager, st));
            OGL_TRY(upload(F.gs_b, gb, 0, reg->stager, st));
            F.gs_pat_id = pat_id;
        }
        if (need_w) {  // W_L and W_U = its transpose: CSR arrays padded like the system matrix, compressed where they qualify
            IsaiPart &W = F.w;
            F.w_pat_id = 0;
            const int32_t N = pat.n_rows;
            const bool sort_w = knob<Knob::isaiSortRows>() != 0.0;
            auto compress = [&](SellDev &d, const std::vector<int32_t> &rp, const std::vector<int32_t> &c) -> int {
                d.ready = false;
                if (!cfg.compress_indices) return OGL_OK;
                OGL_TRY(d.build(N, rp.data(), c.data(), reg->stager, st));
                if (!d.ready && sort_w) OGL_TRY(d.build(N, rp.data(), c.data(), reg->stager, st, true));
                return OGL_OK;
            };
            const size_t wn = w_c.size();
            OGL_TRY(upload(W.w_row_ptrs, w_rp, 0, reg->stager, st));
            OGL_TRY(upload(W.w_cols, w_c, NNZ_PAD, reg->stager, st));
            OGL_TRY(W.w_vals.alloc(wn + NNZ_PAD, st));
            OGL_TRY(upload(W.wt_row_ptrs, wt_rp, 0, reg->stager, st));
            OGL_TRY(upload(W.wt_cols, wt_c, NNZ_PAD, reg->stager, st));
            OGL_TRY(upload(W.wt_map, wt_m, NNZ_PAD, reg->stager, st));
            OGL_TRY(W.wt_vals.alloc(wn + NNZ_PAD, st));
            OGL_TRY(compress(W.w_sell, w_rp, w_c));
            OGL_TRY(compress(W.wt_sell, wt_rp, wt_c));
            W.w_nnz = (int32_t)wn;
            F.w_power = power;
            F.w_ic = ic;
            F.w_pat_id = pat_id;
        }
    }
    if (!want_isai) F.release_isai();  // (switched back to exact: W goes)
    if (sweeps == 0) F.release_sweeps();
    F.tri_isai = want_isai;
    F.sweeps = sweeps;
    OGL_HIP_CHECK(hipMemsetAsync(F.breakdown.p, 0x7f, sizeof(int32_t), st));
    const DevFactor V = F.factor_view();
    if (sweeps > 0) {
        // the factor from `sweeps` synchronous sweeps between two buffers, the last one into F.vals: one launch each
        OGL_TRY(F.a_vals.alloc(std::max<size_t>(1, (size_t)F.nnz), st));
        OGL_TRY(F.sw_vals.alloc(std::max<size_t>(1, (size_t)F.nnz), st));
        launch_factor_gather(st, F.nnz, F.map_ptr.p, F.map.p, csr().vals, F.a_vals.p);
        double *cur = sweeps % 2 == 0 ? F.vals.p : F.sw_vals.p, *other = sweeps % 2 == 0 ? F.sw_vals.p : F.vals.p;
        launch_factor_sweep_start(st, V, F.a_vals.p, cur);
        for (int k = 1; k <= sweeps; ++k) {
            launch_factor_sweep(st, V, F.gs_ptr.p, F.gs_a.p, F.gs_b.p, F.a_vals.p, cur, other, k == sweeps);
            std::swap(cur, other);
        }
    } else {
        // runs of levels of at most iluThinRows rows each: one single-workgroup launch per run
        std::vector<int32_t> seg;
        factor_segments(F.fwd_ptr_h, (int32_t)knob<Knob::iluThinRows>(), seg);
        launch_factor_gather(st, F.nnz, F.map_ptr.p, F.map.p, csr().vals, F.vals.p);
        for (size_t g = 0; g + 2 < seg.size(); g += 3)
            launch_factor_levels(st, V, F.fwd_ptr_h.data(), F.fwd_ptr.p, F.fwd_rows.p, seg[g], seg[g + 1], seg[g + 2] != 0);
    }
    if (ic) launch_gather_coeffs(st, F.nnz, F.t_map.p, F.vals.p, F.t_vals.p);
    if (cfg.preconditioner == OGL_PRECOND_IRILU) {
        OGL_TRY(F.inv_d.alloc((size_t)pat.n_rows + 2, st));
        launch_factor_inv_diag(st, pat.n_rows, F.diag.p, F.vals.p, F.inv_d.p);
    }
    if (want_isai) {
        // W_L from L by substitution over each row's pattern; W_U = W_L^T (IC: gathered, nothing solved twice) or from U
        IsaiPart &W = F.w;
        launch_factor_isai_generate(st, F.n_rows, F.lower(), W.w_row_ptrs.p, W.w_cols.p, W.w_vals.p);
        if (ic) launch_gather_coeffs(st, W.w_nnz, W.wt_map.p, W.w_vals.p, W.wt_vals.p);
        else launch_factor_isai_generate(st, F.n_rows, F.upper(), W.wt_row_ptrs.p, W.wt_cols.p, W.wt_vals.p);
        W.w_sell.refresh(W.w_vals.p, st);
        W.wt_sell.refresh(W.wt_vals.p, st);
    }
    return OGL_OK;
}

// IC / ILU: exact solves y = L^-1 r, z = U^-1 y (U = L^T for IC) level by level; IRILU: 5 Richardson sweeps per
// triangle, x0 = the right-hand side ([UPSTREAM] Ilu<Ir, Ir> with BJ(1) inner solvers, Preconditioner.H:147-178).
// On a renumbered device copy the vectors are carried into the caller's order and back.
void ogl_solver::apply_factor(const double *in, double *out, const DevScalars *gate, double *dot_part)
{
    hipStream_t st = reg->stream;
    const FactorPart &F = precond_data->fac;
    const int32_t n = pat.n_rows;
    const bool rn = pat.renumbered();
    const int32_t *perm = rn ? d_new_id.p : nullptr;
    const DevTri L = F.lower(), U = F.upper();
    if (F.tri_isai) {
        // keyword triangularSolves isai: y = W_L r, z = W_U y through the product kernels and layouts of ISAI's W / W^T
        // (streamed past the caches exactly when the system matrix is); W lives in the caller's numbering
        const bool stream_w = knob<Knob::spmvStream>() == 1.0;
        const IsaiPart &W = F.w;
        const double *r = in;
        double *y = d_fac_tmp[0].p, *z = rn ? d_fac_tmp[1].p : out;
        if (rn) {
            launch_factor_gather_perm(st, n, perm, in, d_fac_tmp[2].p, gate);
            r = d_fac_tmp[2].p;
        }
        SpmvDots last{};
        if (dot_part && !rn) {  // (the last product also leaves the partials of r . z)
            last.with = in;
            last.part = dot_part;
        }
        if (cfg.compress_indices && W.w_sell.ready)
            launch_spmv_sell(st, W.w_sell.view(n, stream_w), SPMV_PLAIN, r, nullptr, y, SpmvDots{}, gate);
        else
            launch_spmv(st, W.w_view(n, stream_w), SPMV_PLAIN, r, nullptr, y, SpmvDots{}, gate);
        if (cfg.compress_indices && W.wt_sell.ready)
            launch_spmv_sell(st, W.wt_sell.view(n, stream_w), SPMV_PLAIN, y, nullptr, z, last, gate);
        else
            launch_spmv(st, W.wt_view(n, stream_w), SPMV_PLAIN, y, nullptr, z, last, gate);
        if (rn) {
            launch_factor_scatter_perm(st, n, perm, z, out, gate);
            if (dot_part) launch_partials_dot(st, n, in, out, dot_part, gate);
        }
        return;
    }
    if (precond_data->kind == PrecondKind::Irilu) {
        constexpr int sweeps = IRILU_SWEEPS;
        const double *b = in;
        if (rn) {
            launch_factor_gather_perm(st, n, perm, in, d_fac_tmp[2].p, gate);
            b = d_fac_tmp[2].p;
        }
        // L (unit diagonal): from x0 = b, the last sweep lands in tmp0
        const double *x = b;
        for (int k = 0; k < sweeps; ++k) {
            double *dst = (sweeps - 1 - k) % 2 == 0 ? d_fac_tmp[0].p : d_fac_tmp[1].p;
            launch_tri_sweep(st, n, L, nullptr, b, x, dst, gate);
            x = dst;
        }
        // U: from x0 = y (tmp0), the last sweep lands in the result (caller's order)
        double *fin = rn ? d_fac_tmp[2].p : out;
        const double *y = d_fac_tmp[0].p;
        x = y;
        for (int k = 0; k < sweeps; ++k) {
            double *dst = (sweeps - 1 - k) % 2 == 0 ? fin : d_fac_tmp[1].p;
            launch_tri_sweep(st, n, U, F.inv_d.p, y, x, dst, gate);
            x = dst;
        }
        if (rn) launch_factor_scatter_perm(st, n, perm, fin, out, gate);
    } else {
        double *x = rn ? d_fac_tmp[2].p : out;
        const std::vector<int32_t> &sf = fac_seg_fwd, &sb = fac_seg_bwd;
        for (size_t g = 0; g + 2 < sf.size(); g += 3)
            launch_tri_levels(st, L, F.fwd_ptr_h.data(), F.fwd_ptr.p, F.fwd_rows.p, sf[g], sf[g + 1], sf[g + 2] != 0, in, perm,
                              x, gate);
        for (size_t g = 0; g + 2 < sb.size(); g += 3)  // (in place: row i reads its own y_i first)
            launch_tri_levels(st, U, F.bwd_ptr_h.data(), F.bwd_ptr.p, F.bwd_rows.p, sb[g], sb[g + 1], sb[g + 2] != 0, x, nullptr,
                              x, gate);
        if (rn) launch_factor_scatter_perm(st, n, perm, x, out, gate);
    }
    if (dot_part) launch_partials_dot(st, n, in, out, dot_part, gate);
}

// Keywords triangularSolves (property 0 exact | 1 isai) and factorSweeps (property 0 .. 10) of IC, ILU and IRILU; every
// other preconditioner ignores them.
int ogl_solver::check_factor_keywords()
{
    OGL_TRY(check_knob(Knob::triangularSolves));
    OGL_TRY(check_knob(Knob::factorSweeps));
    const double tri = knob<Knob::triangularSolves>();
    if (tri == 1.0 && cfg.preconditioner == OGL_PRECOND_IRILU)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner IRILU with triangularSolves isai: IRILU has its own sweeps for the "
                    "triangular solves (use IC or ILU)");
    if (tri == 1.0 && (cfg.sparsity_power < 1 || cfg.sparsity_power > 8))
        return fail(OGL_ERR_INVALID, "triangularSolves isai: sparsityPower %d outside [1, 8]", cfg.sparsity_power);
    return OGL_OK;
}

// where the final scalars take the breakdown word of the preconditioner in use from (nullptr: the kind has none)
const int32_t *ogl_solver::precond_breakdown_word() const
{
    if (!precond_data) return nullptr;
    if (precond_data->factor()) return precond_data->fac.breakdown.p;
    if (precond_data->chebyshev()) return &precond_data->cheb.table.p->breakdown;
    return nullptr;
}

// Chebyshev: a bound that is not finite or not positive (a zero diagonal) fails the solve; `word` as it came back with the
// final scalars.  The solve is over: the bounds in use are read back for the reports here, not in the generation.
int ogl_solver::check_chebyshev_breakdown(int32_t word)
{
    if (!precond_data || !precond_data->chebyshev()) return OGL_OK;
    double bounds[2] = {0.0, 0.0};
    OGL_HIP_CHECK(hipMemcpy(bounds, precond_data->cheb.table.p, sizeof(bounds), hipMemcpyDeviceToHost));
    props["chebyshevLambdaMaxInUse"] = bounds[0];
    props["chebyshevLambdaMinInUse"] = bounds[1];
    if (word == 0) return OGL_OK;
    return fail(OGL_ERR_INVALID, "preconditioner Chebyshev: the bound lambda_max = %g of D^-1 A of the local matrix is not "
                "finite and positive (a zero diagonal entry?)", bounds[0]);
}

// a zero (ILU) / non-positive (IC) pivot of the factor in use: the solve fails instead of handing out NaN.  `word` = the
// factor's breakdown word as it came back with the final scalars.  Several ranks: a breakdown on any rank fails every rank
// (its NaN reaches the others through the all-reduced dots).
int ogl_solver::check_factor_breakdown(int32_t word)
{
    if (!precond_data || !precond_data->factor()) return OGL_OK;
    const int32_t row = word == 0x7f7f7f7f ? -1 : word;
    props["iluBreakdownRow"] = (double)row;
    const bool ic = precond_data->kind == PrecondKind::Ic;
    const char *name = precond_name(precond_data->kind);
    bool elsewhere = false;
    if (reg->comm->multi()) {
        hipStream_t st = reg->stream;
        OGL_TRY(d_flag.alloc(2, st));
        const double mine = row >= 0 ? 1.0 : 0.0;
        double any = 0.0;
        OGL_HIP_CHECK(hipMemcpyAsync(d_flag.p, &mine, sizeof(double), hipMemcpyHostToDevice, st));
        OGL_TRY(reg->allreduce(d_flag.p, 1));
        OGL_HIP_CHECK(hipMemcpyAsync(&any, d_flag.p, sizeof(double), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        elsewhere = any != 0.0 && row < 0;
    }
    if (elsewhere)
        return fail(OGL_ERR_INVALID, "preconditioner %s: the factor of another rank's local matrix broke down", name);
    if (row < 0) return OGL_OK;
    return fail(OGL_ERR_INVALID, "preconditioner %s: %s pivot in row %d of the local matrix (caller's numbering)%s",
                name, ic ? "non-positive" : "zero", row, ic ? " (IC needs a positive diagonal)" : "");
}

void ogl_solver::apply_preconditioner(const double *in, double *out, const DevScalars *gate,
                                      double *dot_part)
{
    hipStream_t st = reg->stream;
    const PrecondData &P = *precond_data;
    const int32_t n = pat.n_rows;
    // the last kernel of the apply also leaves the partials of in . out
    SpmvDots last{};
    if (dot_part) {
        last.with = in;
        last.part = dot_part;
    }
    switch (P.kind) {
    case PrecondKind::None: return;
    case PrecondKind::Jacobi:
        launch_mul(st, n, out, in, P.bj.values.p, gate);
        if (dot_part) launch_partials_dot(st, n, in, out, dot_part, gate);
        return;
    case PrecondKind::Ic:
    case PrecondKind::Ilu:
    case PrecondKind::Irilu: apply_factor(in, out, gate, dot_part); return;
    case PrecondKind::Multigrid: apply_multigrid(in, out, gate, dot_part); return;
    case PrecondKind::Chebyshev: apply_chebyshev(in, out, gate, dot_part); return;
    case PrecondKind::Isai:
    case PrecondKind::Gisai: {  // one or two SpMVs
        const IsaiPart &I = P.isai;
        const bool general = P.kind == PrecondKind::Gisai;
        double *w_out = general ? out : d_isai_tmp.p;
        // (W / W^T are streamed past the caches exactly when the system matrix is: one working set, one policy)
        const bool stream_w = knob<Knob::spmvStream>() == 1.0;
        if (cfg.compress_indices && I.w_sell.ready)
            launch_spmv_sell(st, I.w_sell.view(n, stream_w), SPMV_PLAIN, in, nullptr, w_out, general ? last : SpmvDots{}, gate);
        else
            launch_spmv(st, I.w_view(n, stream_w), SPMV_PLAIN, in, nullptr, w_out, general ? last : SpmvDots{}, gate);
        if (general) return;
        if (cfg.compress_indices && I.wt_sell.ready)
            launch_spmv_sell(st, I.wt_sell.view(n, stream_w), SPMV_PLAIN, d_isai_tmp.p, nullptr, out, last, gate);
        else
            launch_spmv(st, I.wt_view(n, stream_w), SPMV_PLAIN, d_isai_tmp.p, nullptr, out, last, gate);
        return;
    }
    case PrecondKind::BlockJacobi: {
        // (blocks kept in the caller's order -- also a stored object that a field WITHOUT a numbering of its own
        //  generated -- are reached through this solver's permutation)
        const bool perm = pat.renumbered() && (P.bj.through_perm || P.caller_order_blocks());
        const DevBlockJacobi J = P.bj.view(n, P.stride, perm ? d_new_id.p : nullptr, perm ? d_old_of.p : nullptr,
                                           perm ? (int32_t)knob<Knob::bjPermXcdGroup>() : 0);
        if (perm && !P.bj.by_device_row) {
            // (property bjFusedPerm 0: the three-launch form with two staging vectors, for A/B)
            const bool fused_perm = knob<Knob::bjFusedPerm>() != 0.0 && in != out;
            launch_bj_apply_staged(st, J, in, out, dot_part, gate, fused_perm ? nullptr : d_bj_tmp0.p,
                                   fused_perm ? nullptr : d_bj_tmp1.p);
            return;
        }
        launch_bj_apply(st, J, in, out, dot_part, gate);
        return;
    }
    }
}

// This solver's side of an apply of precond_data: the scratch vectors (also for a stored object another field generated)
// and, for the factors, the launch schedule under this solver's own iluThinRows.
int ogl_solver::prepare_apply()
{
    hipStream_t st = reg->stream;
    const PrecondData &P = *precond_data;
    const size_t n = (size_t)pat.n_rows + 2;
    switch (P.kind) {
    case PrecondKind::None:
    case PrecondKind::Gisai: break;
    // (Multigrid's vectors in the caller's order belong to the hierarchy; coarseVisits and its guard are this solver's)
    case PrecondKind::Multigrid: OGL_TRY(prepare_multigrid_apply()); break;
    case PrecondKind::Jacobi: precond = P.bj.values.p; break;
    case PrecondKind::Chebyshev:
        // the second iterate; the unfused step's t = r - A z (released again when this solver's applies run fused)
        cheb_fused = keyword<ChebKeyword::chebyshevFused>() != 0.0 && spmv_layout == SpmvLayout::Sym;
        OGL_TRY(d_cheb_tmp[0].alloc(n, st));
        if (cheb_fused) d_cheb_tmp[1].release();
        else OGL_TRY(d_cheb_tmp[1].alloc(n, st));
        props["chebyshevFusedInUse"] = cheb_fused ? 1.0 : 0.0;
        props["chebyshevLaunchesPerApply"] = (double)(cheb_fused ? P.cheb.degree + 1 : 2 * P.cheb.degree + 1);
        break;
    case PrecondKind::Isai: OGL_TRY(d_isai_tmp.alloc(n, st)); break;  // W r before W^T
    case PrecondKind::BlockJacobi:
        // the staged apply's two vectors in the caller's order
        if (pat.renumbered() && !P.bj.by_device_row && (P.bj.through_perm || P.caller_order_blocks())) {
            OGL_TRY(d_bj_tmp0.alloc(n, st));
            OGL_TRY(d_bj_tmp1.alloc(n, st));
        }
        break;
    case PrecondKind::Ic:
    case PrecondKind::Ilu:
    case PrecondKind::Irilu: {
        // vectors in the caller's order (renumbered) and IRILU's iterates
        const bool irilu = P.kind == PrecondKind::Irilu;
        const bool tri_isai = P.fac.tri_isai;  // (of the object: it is applied the way it was generated)
        if (irilu) {
            OGL_TRY(d_fac_tmp[0].alloc(n, st));
            OGL_TRY(d_fac_tmp[1].alloc(n, st));
        }
        if (tri_isai) {  // y = W_L r, and z in the caller's order on a renumbered copy
            OGL_TRY(d_fac_tmp[0].alloc(n, st));
            if (pat.renumbered()) OGL_TRY(d_fac_tmp[1].alloc(n, st));
        } else if (fac_isai_scratch && !irilu) {  // (back on the exact solves: the scratch of the products goes)
            d_fac_tmp[0].release();
            d_fac_tmp[1].release();
        }
        fac_isai_scratch = tri_isai;
        if (pat.renumbered()) OGL_TRY(d_fac_tmp[2].alloc(n, st));
        const int32_t thin = (int32_t)knob<Knob::iluThinRows>();
        factor_segments(P.fac.fwd_ptr_h, thin, fac_seg_fwd);
        factor_segments(P.fac.bwd_ptr_h, thin, fac_seg_bwd);
        int launches = 0;
        if (tri_isai) {
            launches = 2 + (pat.renumbered() ? 2 : 0);
        } else if (irilu) {
            launches = 2 * IRILU_SWEEPS + (pat.renumbered() ? 2 : 0);
        } else {
            for (const std::vector<int32_t> *seg : {&fac_seg_fwd, &fac_seg_bwd})
                for (size_t g = 0; g + 2 < seg->size(); g += 3) launches += (*seg)[g + 2] ? 1 : (*seg)[g + 1] - (*seg)[g];
            launches += pat.renumbered() ? 1 : 0;
        }
        props["iluLevels"] = (double)(P.fac.fwd_ptr_h.size() - 1);
        props["iluLaunchesPerApply"] = (double)launches;  // (without the fused dot of a Krylov turn)
        props["triangularSolvesInUse"] = tri_isai ? 1.0 : 0.0;
        props["triangularWEntries"] = tri_isai ? (double)P.fac.w.w_nnz : 0.0;
        props["factorSweepsInUse"] = (double)P.fac.sweeps;
        break;
    }
    }
    return OGL_OK;
}

// ------------------------------------------------------------------------------------------
// Preconditioner::init_preconditioner (Preconditioner.H:353-431) with its caching rules:
//   * nothing stored yet      -> generate, store, counter := caching
//   * stored and counter > 0  -> counter -= 1, use the STORED one
//   * stored and counter == 0 -> counter := caching, generate a fresh one for this solve only;
//                                the stored object is not replaced (:411-413)
// The store is registry-wide (one key for all fields, :357), as in the reference.
// ------------------------------------------------------------------------------------------
int ogl_solver::init_preconditioner()
{
    precond = nullptr;
    precond_data = nullptr;
    precond_ready = false;
    if (cfg.preconditioner == OGL_PRECOND_NONE) {  // :342
        precond_ready = true;
        precond_pat = pat_id;
        return OGL_OK;
    }
    const PrecondKind kind = precond_kind_of(cfg);
    const bool isai = is_isai(kind);
    if (kind == PrecondKind::Multigrid) OGL_TRY(check_multigrid_keywords());
    if (kind == PrecondKind::None)
        return fail(OGL_ERR_UNSUPPORTED, "preconditioner kind %d is not built", cfg.preconditioner);
    if (isai && (cfg.sparsity_power < 1 || cfg.sparsity_power > 8))
        return fail(OGL_ERR_INVALID, "ISAI sparsityPower %d outside [1, 8]", cfg.sparsity_power);
    if (cfg.preconditioner == OGL_PRECOND_BJ && (cfg.max_block_size < 1 || cfg.max_block_size > MAX_JACOBI_BLOCK))
        return fail(OGL_ERR_INVALID, "BJ maxBlockSize %d outside [1, %d]", cfg.max_block_size,
                    MAX_JACOBI_BLOCK);
    if (is_factor(kind)) OGL_TRY(check_factor_keywords());
    if (kind == PrecondKind::Chebyshev) OGL_TRY(check_chebyshev_keywords());
    const int stride = precond_stride(kind);
    const int cache = (int)knob<Knob::preconditionerCaching>();
    const bool stored =
        reg->has_cached_precond && reg->cached_precond.matches(kind, (size_t)pat.n_rows, stride);
    // (the store is shared by all fields, Preconditioner.H:357: a stored object whose values live in ANOTHER pattern's
    //  device numbering would be a silently permuted operator here: generate for this solve instead.  The table:
    //  PrecondData::foreign_to)
    const bool foreign = stored && reg->cached_precond.foreign_to(pat_id, pat.renumbered());
    // (property precondTimedApplies > 0, measurements only: the generation and that many applies timed with HIP events)
    const int timed = (int)knob<Knob::precondTimedApplies>();
    EventPair tev;
    if (timed > 0) {
        OGL_HIP_CHECK(ev_create(&tev[0]));
        OGL_HIP_CHECK(ev_create(&tev[1]));
    }
    if (stored && cache > 0 && !foreign) {
        set_knob<Knob::preconditionerCaching>(cache - 1);
        precond_data = &reg->cached_precond;
    } else {
        set_knob<Knob::preconditionerCaching>(cfg.caching);
        PrecondData &P = stored ? own_precond : reg->cached_precond;
        if (timed > 0) OGL_HIP_CHECK(hipEventRecord(tev[0], reg->stream));
        OGL_TRY(generate_preconditioner(P));
        if (timed > 0) {
            OGL_HIP_CHECK(hipEventRecord(tev[1], reg->stream));
            OGL_HIP_CHECK(hipEventSynchronize(tev[1]));
            float ms = 0.f;
            OGL_HIP_CHECK(hipEventElapsedTime(&ms, tev[0], tev[1]));
            props["precondGenerateMs"] = ms;
        }
        if (!stored) reg->has_cached_precond = true;
        precond_data = &P;
    }
    OGL_TRY(prepare_apply());
    if (timed > 0 && d_w.p && d_q.p) {
        OGL_HIP_CHECK(hipEventRecord(tev[0], reg->stream));
        for (int i = 0; i < timed; ++i) apply_preconditioner(d_w.p, d_q.p, nullptr);
        OGL_HIP_CHECK(hipEventRecord(tev[1], reg->stream));
        OGL_HIP_CHECK(hipEventSynchronize(tev[1]));
        float ms = 0.f;
        OGL_HIP_CHECK(hipEventElapsedTime(&ms, tev[0], tev[1]));
        props["precondApplyMs"] = ms / timed;
    }
    precond_ready = true;
    precond_serial = precond_data->serial;
    precond_pat = pat_id;
    return OGL_OK;
}

bool ogl_solver::precond_current() const
{
    if (!precond_ready || !matrix_set || precond_pat != pat_id) return false;
    if (!precond_data) return cfg.preconditioner == OGL_PRECOND_NONE;
    return precond_data->serial == precond_serial && precond_data->n_rows == (size_t)pat.n_rows;
}
