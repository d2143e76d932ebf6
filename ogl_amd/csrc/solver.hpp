// solver.hpp -- persistent per-(rank, field) device state and the Krylov drivers.
// Re-implements the reference's L2-L4: DevicePersistent/*, HostMatrixWrapper's
// device half, Preconditioner caching, StoppingCriterion policy and lduLduBase orchestration.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "comm.hpp"
#include "common.hpp"
#include "host_matrix.hpp"
#include "kernels.hpp"
#include "properties.hpp"
#include "setup_kernels.hpp"
#include "spmv_layouts.hpp"

namespace ogl {

// What a level of a Multigrid hierarchy holds once per precision of the cycle: the values (where the level keeps a matrix
// of its own), 1 / diagonal, and the vectors -- right-hand side (levels >= 1), iterates, A x; r, p: the coarsest level's CG.
template <class T>
struct MgOperands {
    DevBuf<T> vals, inv_d;
    DevBuf<T> b, xa, xb, t, r, p;
};

// One matrix of a Multigrid hierarchy with what its V-cycle needs (kernels_mg.hip).  Level 0 is the system matrix itself:
// it keeps no copy of it, only 1 / diagonal, the aggregates and the vectors.
struct MgLevel {
    int32_t n = 0, nnz = 0, n_coarse = 0;      // n_coarse: rows of the next level (0: this is the coarsest)
    int passes = 0;                            // pairwise coarsenings that made the next level (aggregatePasses; 0: coarsest)
    // levels >= 1; level 0 only on a renumbered device copy (own: the system matrix in the CALLER's numbering, in which
    // the hierarchy lives -- the products then run on it instead of the in-loop layout)
    bool own = true;
    DevBuf<int32_t> row_ptrs, cols;
    DevBuf<int32_t> agg, agg_ptr, agg_rows;    // fine-to-coarse map, members per coarse row (ascending)
    DevBuf<double> part;                       // the per-chunk partials of the coarsest CG's sums (doubles in either precision)
    // keyword aggregateCaching: per pass that made the next level, what a refresh of its values reads (kernels.hpp,
    // launch_mg_regalerkin) -- src over the pass's source entries, ptr over its kept_nnz coarse entries (+ 1).  Left by a
    // full generation that was asked to; they only grow.
    DevBuf<int32_t> kept_src[MG_MAX_PASSES], kept_ptr[MG_MAX_PASSES];
    int32_t kept_nnz[MG_MAX_PASSES] = {};
    size_t kept_bytes() const
    {
        size_t bytes = 0;
        for (int p = 0; p < MG_MAX_PASSES; ++p) bytes += (kept_src[p].cap + kept_ptr[p].cap) * sizeof(int32_t);
        return bytes;
    }
    // dbl: what the generation makes.  flt (keyword cyclePrecision single): the binary32 twin -- values
    // and 1 / d rounded from dbl's, on the same index arrays -- and the level's vectors in binary32.  Built by the first
    // apply in single precision of a generated hierarchy (MultigridPart::twin_of); they only grow.
    MgOperands<double> dbl;
    MgOperands<float> flt;
    template <class T>
    const MgOperands<T> &ops() const
    {
        if constexpr (std::is_same<T, double>::value) return dbl;
        else return flt;
    }
    template <class T>
    MgCsrOf<T> view() const { return MgCsrOf<T>{n, nnz, row_ptrs.p, cols.p, ops<T>().vals.p}; }
};

// One apply of a hierarchy as the steps of its cycle see it: the gate of every launch, and how many there were (property
// mgLaunchesPerApply).  A step gets the stream of a launch from next(), which counts it: the count is kept where the
// launches are made.
struct MgRun {
    hipStream_t st = nullptr;
    const DevScalars *gate = nullptr;
    int launches = 0;
    hipStream_t next() { return ++launches, st; }
};
// The fp64 ends of the cycle in single precision: level 0 reads the residual from `in` and writes z to `out` as doubles.
// Empty for every other level, and in double precision (where level 0's b and x are those vectors themselves).
struct MgWide {
    const double *in = nullptr;
    double *out = nullptr;
};

// The preconditioner kinds.  precond_kind_of is the only place that turns the configuration (the public OGL_PRECOND_*
// value + maxBlockSize) into one, precond_name the only place that holds the names the error messages use.
enum class PrecondKind { None, Jacobi, BlockJacobi, Isai, Gisai, Ic, Ilu, Irilu, Multigrid, Chebyshev };
inline PrecondKind precond_kind_of(const ogl_config &cfg)  // (None also for a value that is not built)
{
    switch (cfg.preconditioner) {
    case OGL_PRECOND_BJ: return cfg.max_block_size == 1 ? PrecondKind::Jacobi : PrecondKind::BlockJacobi;
    case OGL_PRECOND_ISAI: return PrecondKind::Isai;
    case OGL_PRECOND_GISAI: return PrecondKind::Gisai;
    case OGL_PRECOND_IC: return PrecondKind::Ic;
    case OGL_PRECOND_ILU: return PrecondKind::Ilu;
    case OGL_PRECOND_IRILU: return PrecondKind::Irilu;
    case OGL_PRECOND_MULTIGRID: return PrecondKind::Multigrid;
    case OGL_PRECOND_CHEBYSHEV: return PrecondKind::Chebyshev;
    default: return PrecondKind::None;
    }
}
inline const char *precond_name(PrecondKind k)
{
    static const char *const names[] = {"none", "BJ", "BJ", "ISAI", "GISAI", "IC", "ILU", "IRILU", "Multigrid", "Chebyshev"};
    return names[(int)k];
}
inline bool is_isai(PrecondKind k) { return k == PrecondKind::Isai || k == PrecondKind::Gisai; }
inline bool is_factor(PrecondKind k) { return k == PrecondKind::Ic || k == PrecondKind::Ilu || k == PrecondKind::Irilu; }

// ---- what each kind owns: its buffers, its pattern-only record, and the views its kernels take (kernels.hpp) ----

// Block Jacobi: the inverted blocks.  Scalar Jacobi keeps its inverse diagonal (n_rows + 2) in `values` too.
struct BlockJacobiPart {
    int32_t n_blocks = 0;
    bool uniform_blocks = false;  // every block but the last has exactly `stride` rows
    bool through_perm = false;    // block_ptrs / row_block are positions in the caller's numbering
    uint64_t perm_pat_id = 0;     // ... of THIS pattern's permutation
    bool by_device_row = false;   // block rows stored at their device rows (direct apply) instead of block-major (staged)
    DevBuf<double> values;
    DevBuf<int32_t> block_ptrs, row_block;
    void release()
    {
        values.release();
        block_ptrs.release();
        row_block.release();
    }
    // rows / pos: the permutation the blocks are reached through (the generating or the applying solver's), or nullptr
    DevBlockJacobi view(int32_t n_rows, int stride, const int32_t *rows, const int32_t *pos, int32_t perm_xcd_group = 0) const
    {
        DevBlockJacobi J;
        J.n_rows = n_rows;
        J.n_blocks = n_blocks;
        J.stride = stride;
        J.block_ptrs = block_ptrs.p;
        J.row_block = row_block.p;
        J.blocks = values.p;
        J.uniform = uniform_blocks ? 1 : 0;
        J.rows = rows;
        J.pos = pos;
        J.by_device_row = rows && by_device_row ? 1 : 0;
        J.perm_xcd_group = perm_xcd_group;
        return J;
    }
};

// ISAI (spd, M^-1 = W^T W) and GISAI (general, M^-1 = W): CSR arrays padded like the system matrix so the CSR-stream
// SpMV kernel applies them; wt_map = position in W of every entry of W^T (IsaiStructure, host_matrix.hpp)
struct IsaiPart {
    DevBuf<int32_t> w_row_ptrs, w_cols, wt_row_ptrs, wt_cols, wt_map;
    DevBuf<double> w_vals, wt_vals;
    int32_t w_nnz = 0, w_max_row = 0;
    DevBuf<int32_t> wide_rows;  // rows of W with ISAI_THREAD_ROW < entries <= MAX_ISAI_ROW (one wavefront each)
    int32_t n_wide_rows = 0;
    // rows of W with more than MAX_ISAI_ROW entries (one workgroup each, dense system in global scratch):
    // huge_off[k] = start of row huge_rows[k]'s system in huge_scratch; huge_batches = runs of rows that share
    // the scratch at one time
    DevBuf<int32_t> huge_rows;
    DevBuf<int64_t> huge_off;
    DevBuf<double> huge_scratch;  // allocated for a generation, released after it
    int64_t huge_scratch_len = 0;
    std::vector<int32_t> huge_batches;
    int32_t n_huge_rows = 0;
    SellDev w_sell, wt_sell;  // compressed copies the apply runs on when compress_indices is set
    void release()
    {
        for (DevBuf<int32_t> *b : {&w_row_ptrs, &w_cols, &wt_row_ptrs, &wt_cols, &wt_map, &wide_rows, &huge_rows}) b->release();
        for (DevBuf<double> *b : {&w_vals, &wt_vals, &huge_scratch}) b->release();
        huge_off.release();
        w_sell.release();
        wt_sell.release();
    }
    DevCsr w_view(int32_t n_rows, bool stream) const { return csr_view(n_rows, stream, w_row_ptrs, w_cols, w_vals); }
    DevCsr wt_view(int32_t n_rows, bool stream) const { return csr_view(n_rows, stream, wt_row_ptrs, wt_cols, wt_vals); }

private:
    DevCsr csr_view(int32_t n_rows, bool stream, const DevBuf<int32_t> &rp, const DevBuf<int32_t> &c,
                    const DevBuf<double> &v) const
    {
        DevCsr W;
        W.n_rows = n_rows;
        W.nnz = w_nnz;
        W.row_ptrs = rp.p;
        W.cols = c.p;
        W.vals = v.p;
        W.stream = stream;
        return W;
    }
};

// Incomplete factorisations (IC, ILU, IRILU; FactorStructure, host_matrix.hpp): the factor in the CALLER's numbering --
// self-contained, applied through the applying solver's permutation -- with its value map, update lists, L^T (IC) and
// the level schedules.  ILU and IRILU share the factor.
struct FactorPart {
    int32_t n_rows = 0, nnz = 0;
    bool ic = false;
    DevBuf<int32_t> row_ptrs, cols, diag, map_ptr, map, upd_ptr, upd_a, upd_b;
    DevBuf<int32_t> t_row_ptrs, t_cols, t_map, fwd_ptr, fwd_rows, bwd_ptr, bwd_rows;
    DevBuf<double> vals, t_vals, inv_d;
    DevBuf<int32_t> breakdown;  // first row with a zero / non-positive pivot (0x7f7f7f7f: none)
    std::vector<int32_t> fwd_ptr_h, bwd_ptr_h;
    // keyword factorSweeps N (what this object was generated with): the gathered values of A, the second buffer of the
    // sweeps, and ILU's update pairs in gather form, built for pattern gs_pat_id
    int sweeps = 0;
    DevBuf<double> a_vals, sw_vals;
    DevBuf<int32_t> gs_ptr, gs_a, gs_b;
    uint64_t gs_pat_id = 0;
    // keyword triangularSolves isai (what this object was generated with): W_L in w.w_*, W_U in w.wt_* (IC: gathered
    // through wt_map), both in the caller's numbering, their pattern built for (w_pat_id, w_power, w_ic)
    bool tri_isai = false;
    IsaiPart w;
    uint64_t w_pat_id = 0;
    int w_power = 0;
    bool w_ic = false;
    void release_sweeps()
    {
        for (DevBuf<int32_t> *b : {&gs_ptr, &gs_a, &gs_b}) b->release();
        for (DevBuf<double> *b : {&a_vals, &sw_vals}) b->release();
        gs_pat_id = 0;
    }
    void release_isai()
    {
        w.release();
        w_pat_id = 0;
    }
    void release()
    {
        for (DevBuf<int32_t> *b : {&row_ptrs, &cols, &diag, &map_ptr, &map, &upd_ptr, &upd_a, &upd_b, &t_row_ptrs, &t_cols, &t_map,
                                   &fwd_ptr, &fwd_rows, &bwd_ptr, &bwd_rows, &breakdown})
            b->release();
        for (DevBuf<double> *b : {&vals, &t_vals, &inv_d}) b->release();
        release_sweeps();
        release_isai();
    }
    DevFactor factor_view() const
    {
        DevFactor F;
        F.n_rows = n_rows;
        F.ic = ic ? 1 : 0;
        F.row_ptrs = row_ptrs.p;
        F.cols = cols.p;
        F.diag = diag.p;
        F.vals = vals.p;
        F.upd_ptr = upd_ptr.p;
        F.upd_a = upd_a.p;
        F.upd_b = upd_b.p;
        F.breakdown = breakdown.p;
        return F;
    }
    DevTri lower() const  // (ILU: unit diagonal)
    {
        DevTri L;
        L.beg = row_ptrs.p;
        L.end = diag.p;
        L.cols = cols.p;
        L.vals = vals.p;
        L.unit = ic ? 0 : 1;
        return L;
    }
    DevTri upper() const  // (IC: L^T)
    {
        DevTri U;
        U.upper = 1;
        U.beg = ic ? t_row_ptrs.p : diag.p;
        U.end = (ic ? t_row_ptrs.p : row_ptrs.p) + 1;
        U.cols = ic ? t_cols.p : cols.p;
        U.vals = ic ? t_vals.p : vals.p;
        return U;
    }
};

// Multigrid: the levels in use are levels[0 .. n_levels); the objects behind them are kept from generation to
// generation so that their buffers only grow.  The work buffers: what a generation needs besides (also only growing).
struct MultigridPart {
    std::vector<std::unique_ptr<MgLevel>> levels;
    int n_levels = 0, cg_iters = 0;
    DevBuf<MgScalars> scal;
    DevBuf<int32_t> map0;      // renumbered device copy: position in the device CSR of every entry of level 0
    DevBuf<double> in, out;    // ... and the vectors of an apply in the caller's order
    DevBuf<double> diag, vals_sorted;
    DevBuf<int32_t> s, flag, incl, cidx, rows, sorted, left;
    DevBuf<unsigned long long> keys, keys_sorted;
    DevBuf<uint8_t> temp;
    // aggregatePasses > 1: the matrices between two kept levels (one read, one written) and a pass's own aggregation
    DevBuf<int32_t> pass_row_ptrs[2], pass_cols[2], pass_agg;
    DevBuf<double> pass_vals[2];
    // cyclePrecision single: `generated` counts the generations of this object, twin_of names the one the levels' binary32
    // twins were rounded from (0: none); bad: the overflow words of the conversions -- [0] the position in the fine level's
    // fp32 copy (Fp32Dev), [1 + l] the row of level l's twin.  The twin is a cache of the hierarchy, made by whichever
    // solver first applies it in single precision: hence mutable.
    uint64_t generated = 0;
    mutable uint64_t twin_of = 0;
    mutable DevBuf<int32_t> bad;
    // keyword aggregateCaching: what the aggregates of this object were made for (valid: by a full generation that ran to
    // its end and kept the levels' maps), and how many generations may still refresh the values under them.  host_reads:
    // the device-to-host reads of the last generation.
    struct KeptFor {
        bool valid = false;
        uint64_t pat_id = 0;
        int32_t rows = 0, nnz = 0;
        bool own = false, hashed = false;
        int passes = 0, max_levels = 0;
        double min_coarse = 0.0;
        bool operator==(const KeptFor &o) const
        {
            return valid == o.valid && pat_id == o.pat_id && rows == o.rows && nnz == o.nnz && own == o.own &&
                   hashed == o.hashed && passes == o.passes && max_levels == o.max_levels && min_coarse == o.min_coarse;
        }
    } kept_for;
    int kept_left = 0, host_reads = 0;
    size_t kept_bytes() const
    {
        size_t bytes = 0;
        for (const auto &L : levels) bytes += L->kept_bytes();
        return bytes;
    }
    void release()
    {
        levels.clear();
        n_levels = 0;
        twin_of = 0;
        kept_for = KeptFor{};
        kept_left = 0;
        bad.release();
        scal.release();
        for (DevBuf<int32_t> *b : {&map0, &s, &flag, &incl, &cidx, &rows, &sorted, &left, &pass_agg, &pass_row_ptrs[0],
                                   &pass_row_ptrs[1], &pass_cols[0], &pass_cols[1]})
            b->release();
        for (DevBuf<double> *b : {&in, &out, &diag, &vals_sorted, &pass_vals[0], &pass_vals[1]}) b->release();
        keys.release();
        keys_sorted.release();
        temp.release();
    }
};

// Chebyshev: 1 / diagonal (n_rows + 2, scalar Jacobi's bits), the table of the recurrence with the
// breakdown word (ChebTable, kernels.hpp), and the degree the table was written for.  w belongs to the generating
// pattern's device numbering, like scalar Jacobi's inverse diagonal.
struct ChebPart {
    DevBuf<double> w;
    DevBuf<ChebTable> table;
    int degree = 0;
    void release()
    {
        w.release();
        table.release();
    }
};

// A generated preconditioner ("Cached_preconditinoner" holds one of these, Preconditioner.H:357): what is common to all
// kinds, and one part per family of kinds.  All parts are present at all times and the parts of the OTHER kinds are
// NOT released when the object changes kind: the store is registry-wide, so a case with ISAI on p and block Jacobi on
// U alternates kinds with every time step, and no allocation after the first steps is promised.
// That is why the parts are members and not a variant.
struct PrecondData {
    PrecondKind kind = PrecondKind::None;
    size_t n_rows = 0;
    int stride = 0;  // block Jacobi: maxBlockSize; ISAI / GISAI: sparsityPower; Chebyshev: chebyshevDegree
    BlockJacobiPart bj;
    IsaiPart isai;
    FactorPart fac;
    MultigridPart mg;
    ChebPart cheb;
    void release()
    {
        cheb.release();
        bj.release();
        isai.release();
        fac.release();
        mg.release();
    }
    bool materialises_z() const { return kind != PrecondKind::None && kind != PrecondKind::Jacobi; }  // (Jacobi: fused)
    bool is_isai() const { return ogl::is_isai(kind); }
    bool factor() const { return is_factor(kind); }
    bool multigrid() const { return kind == PrecondKind::Multigrid; }
    bool chebyshev() const { return kind == PrecondKind::Chebyshev; }
    uint64_t serial = 0;  // new value with every generation (an applier checks it still holds what it adopted)
    // the pattern-only part (block pointers / W and W^T patterns / the factor's structure / Multigrid's level 0) is kept
    // for as long as it was derived from the same sparsity pattern: only the values are regenerated per solve
    uint64_t struct_pat_id = 0;
    PrecondKind struct_kind = PrecondKind::None;
    int struct_stride = 0;
    bool struct_caller_numbering = true;
    bool has_structure(uint64_t id, PrecondKind k, int st) const
    {
        return id != 0 && struct_pat_id == id && struct_kind == k && struct_stride == st;
    }
    void set_structure(uint64_t id, PrecondKind k, int st)
    {
        struct_pat_id = id;
        struct_kind = k;
        struct_stride = st;
    }
    bool matches(PrecondKind k, size_t n, int st) const { return kind == k && n_rows == n && stride == st; }
    // Which numbering the VALUES are laid out in.  The store is shared by all fields (Preconditioner.H:357), so the
    // object may be applied by a solver other than the one that generated it.  Generated on a renumbered device copy,
    // these keep the caller's order all the same: the factors, a Multigrid hierarchy (it then has a level 0 of its own),
    // and a block Jacobi kept block-major in the caller's order (the applying solver carries the vectors through ITS
    // permutation).  Everything else -- inverse diagonal, W / W^T, block rows stored by device row, the backend's own
    // blocks -- then belongs to the generating pattern's device numbering.
    uint64_t gen_pat_id = 0;
    bool gen_device_numbering = false;
    bool keeps_caller_order() const
    {
        return factor() || multigrid() || (kind == PrecondKind::BlockJacobi && bj.through_perm && !bj.by_device_row);
    }
    bool caller_order_blocks() const
    {
        return kind == PrecondKind::BlockJacobi && !bj.by_device_row && !gen_device_numbering;
    }
    // May a solver with pattern `id` (renumbered or not) apply this object?  Own pattern: always.  Another pattern:
    //
    //   kind                                         generator renumbered   applier renumbered   ->
    //   Jacobi, ISAI, GISAI, Chebyshev               yes                    any                  foreign
    //                                                no                     yes                  foreign
    //                                                no                     no                   own
    //   block Jacobi, block-major in caller's order  any                    any                  own (through the applier's permutation)
    //   block Jacobi, by device row / backend blocks yes                    any                  foreign
    //   IC, ILU, IRILU                               any                    any                  own (through the applier's permutation)
    //   Multigrid                                    any                    yes                  foreign
    //                                                any                    no                   own
    //
    // (a Multigrid hierarchy is self-contained only when its generator kept a level 0 of its own)
    bool foreign_to(uint64_t id, bool renumbered) const
    {
        if (gen_pat_id == id) return false;
        return gen_device_numbering || (renumbered && !caller_order_blocks() && !factor());
    }
};

// Mixed precision for GKOCG (solver_mixed.cpp): the fp32 vectors of the inner solve, the fp32
// inverse diagonal, the scalars of both loops with their pinned poll slots, and a staging vector for ogl_solver_spmv_f32.
// Allocated at the first mixed solve and kept.
struct MixedPart {
    DevBuf<float> u, r, z, p, q, inv_d, io;
    DevBuf<MixedScalars> scal;
    MixedScalars *h_scal = nullptr;  // pinned, 2 slots
    void release()
    {
        for (DevBuf<float> *b : {&u, &r, &z, &p, &q, &inv_d, &io}) b->release();
        scal.release();
        ledger::pinned_free(h_scal);
        h_scal = nullptr;
    }
};

// The initial guess from the last solutions (keyword guessProjection K; solver_proj.cpp): the ring
// of stored steps and W = A D, K vectors of leading dimension ld each, the partials and the small arrays of the pre-step.
// Sized at the first solve with K > 0 and kept.  The stored vectors, oldest first: slots first, first + 1, .. (mod K).
struct ProjPart {
    DevBuf<double> ring, W, part, small;
    int K = 0, count = 0, first = 0;
    int64_t ld = 0;
    uint64_t pat_id = 0;
    // the solve under way: vectors offered, launches of its pre-step, whether a step may be stored after it
    int offered = 0, launches = 0;
    bool active = false;
    bool credit = false;    // keyword guessProjectionCredit 1 on this solve (K > 0)
    bool one_pass = false;  // keyword guessProjectionProducts onePass, and this solve's products ran that way
    hipEvent_t ev[5] = {};  // property guessProjectionTimed: products | Gram pass | small solve | update
    bool timed = false;
    double *slot(int j) const { return ring.p + (size_t)((first + j) % K) * (size_t)ld; }  // stored vector j, oldest first
    double *sums() const { return small.p; }
    double *sums_copy() const { return small.p + 64; }
    double *h() const { return small.p + 128; }
    double *rec() const { return small.p + 144; }
    static constexpr size_t SMALL_LEN = 160;
    void clear() { count = first = 0; }
    void release()
    {
        for (DevBuf<double> *b : {&ring, &W, &part, &small}) b->release();
        for (auto &e : ev)
            if (e) ev_destroy(e);
        for (auto &e : ev) e = nullptr;
        K = 0;
        clear();
    }
};

}  // namespace ogl

struct ogl_solver;

// objectRegistry analogue (DevicePersistent/Base/Base.H:53-137) + ExecutorHandler
struct ogl_registry {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // halo exchange runs on its own stream so that it overlaps the local SpMV (K3)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_received = nullptr;
    std::unique_ptr<ogl::Comm> comm;
    std::map<std::string, std::unique_ptr<ogl_solver>> solvers;
    ogl::Stager stager;
    // "Cached_preconditinoner" (sic) -- one registry-wide slot (Preconditioner.H:357)
    ogl::PrecondData cached_precond;
    bool has_cached_precond = false;
    // Peer-write all-reduce mesh (PeerArgs, kernels.hpp): own mailbox + the other ranks' mailboxes
    // mapped through hipIpc.  When `peer_ready`, the scalar all-reduces run inside the finaliser
    // kernels instead of through comm->allreduce (the halo exchange stays with `comm`).
    unsigned long long *peer_local = nullptr;
    void *peer_mapped[ogl::PEER_MAX_RANKS] = {};  // hipIpcOpenMemHandle results (closed on destroy)
    int32_t *peer_error = nullptr;                // device flag for the stand-alone all-reduce kernel
    ogl::PeerArgs peer{};                         // world/rank/box[]; seq is stamped per call
    uint32_t peer_seq = 0;
    bool peer_ready = false;
    bool peer_shared_device = false;  // two ranks of the mesh report the same PCI bus id (peer_connect)
    // peer-put halo arena behind the mailbox in the same IPC allocation (PeerHalo, kernels.hpp):
    // solvers take blocks at pattern-build time; every rank builds patterns in the same order, so
    // `halo_epoch` names the same handshake on all ranks
    size_t arena_words = 0, arena_used = 0;
    uint32_t halo_epoch = 0;
    int peer_export(void *handle_out);
    int peer_connect(int rank, int n_ranks, const void *handles);
    void peer_close();
    // next all-reduce's arguments (every rank calls this the same number of times, in the same order)
    ogl::PeerArgs peer_next()
    {
        ogl::PeerArgs p = peer;
        if (++peer_seq == 0) ++peer_seq;
        p.seq = peer_seq;
        return p;
    }
    // in-place SUM of n <= 2 doubles over the ranks, on `stream`
    int allreduce(double *dev, int n);
    ~ogl_registry();
};

struct ogl_solver {
    ogl_registry *reg = nullptr;
    std::string field;
    ogl_config cfg{};

    // ---- HostMatrixWrapper state ----
    ogl::HostPattern pat;
    bool have_pattern = false;
    uint64_t pat_id = 0;  // unique per built sparsity pattern (keys the preconditioner structure)
    bool matrix_set = false;
    ogl::DevBuf<int32_t> d_row_ptrs, d_cols, d_ldu_mapping;  // "<field>_local_*"
    ogl::DevBuf<double> d_vals;                              // "<field>_matrix" values
    ogl::DevBuf<double> d_source;                            // unsorted [upper|lower|diag|iface]
    ogl::DevBuf<int32_t> d_diag_pos;  // position of each row's first diagonal entry (scalar Jacobi)
    // ---- derived device layouts the SpMV may run on instead of the CSR arrays (spmv_layouts.hpp) ----
    // matrixFormat Ell; the half storage of a symmetric matrix (compress_indices + symmetric_half), else its per-chunk
    // variant; the index-compressed chunked ELL (compress_indices); the packed columns of the CSR-stream kernel.  Each is
    // built once per pattern and refreshed from d_vals when it is about to be timed or used (refresh_values).
    ogl::EllDev ell_dev;
    ogl::SymDev sym_dev;
    ogl::SymxDev symx_dev;
    ogl::SellDev sell_dev;
    ogl::Stream21Dev s21_dev;
    ogl::Fp32Dev fp32_dev;  // the fp32 copy the mixed-precision inner solve runs on
    uint64_t vals_epoch = 0;  // bumped by every coefficient upload into d_vals
    void refresh_values(ogl::SpmvLayout l);
    void release_layout(ogl::SpmvLayout l);
    // The layout the in-loop SpMV runs on: chosen by select_spmv_layout at the end of every set_matrix (after any
    // timing), Csr from a coefficient or pattern change until then.  The views below are those the kernels get.
    ogl::SpmvLayout spmv_layout = ogl::SpmvLayout::Csr;
    int select_spmv_layout();
    // Patterns with irregular chunks (16-bit delta / 32-bit column codes: unstructured meshes) are timed on the
    // candidate kernels once per pattern (tune_spmv_layouts): the compressed layout moves fewer bytes, but its slot-major
    // gather -- one entry of 64 different rows per instruction -- only pays where neighbouring rows have neighbouring
    // columns; on a polyhedral mesh the CSR-stream kernel's row-major gather wins.  The results are bit-identical.
    bool layout_tuned = false;  // ... done for this pattern
    int tune_spmv_layouts(const std::vector<ogl::SpmvLayout> &cand, const ogl::SpmvLayout *pin, ogl::SpmvLayout *winner);
    // `pre` != nullptr: the layout choose_numbering already derived for this pattern (`pre_qualifies`: usable)
    int build_sell(ogl::SellLayout *pre = nullptr, bool pre_qualifies = false);
    bool band_order_off = std::getenv("OGL_NO_BAND_ORDER") != nullptr;  // (A/B switch for measurements)
    bool streamed(double bytes) const { return bytes + turn_extra_bytes() > stream_above_bytes(); }
    ogl::DevEll ell() const { return ell_dev.view(pat.n_rows, streamed(ell_dev.bytes(pat.n_rows))); }
    ogl::DevSym sym() const { return sym_dev.view(pat.n_rows, streamed(sym_dev.bytes(pat.n_rows)), !band_order_off); }
    ogl::DevSymx symx() const { return symx_dev.view(pat.n_rows, streamed(symx_dev.bytes(pat.n_rows)), xcd_group()); }
    ogl::DevSell sell() const
    {
        return sell_dev.view(pat.n_rows, streamed(sell_dev.bytes(pat.n_rows)), xcd_group(), &d_band_order);
    }
    ogl::DevCsr csr(bool packed) const;  // packed: with the packed columns (SpmvLayout::Csr21)
    ogl::DevCsr csr() const { return csr(spmv_layout == ogl::SpmvLayout::Csr21); }
    // device set-up (setup_kernels.hip)
    int build_pattern_on_device(const ogl_ldu_view &ldu, ogl::HostPattern &np, bool *built);
    int build_sym_on_device(const ogl::HostPattern &np, ogl::SymDistances *sd_out, bool *done);
    int download_local_pattern(ogl::HostPattern &hp);
    // reverse Cuthill-McKee of the device pattern (same order as rcm_order); new_id stays empty when the graph
    // is not one for a level-synchronous search (very many components or levels): the host does it then
    int rcm_on_device(const ogl::HostPattern &hp, std::vector<ogl_label> &new_id);
    // device pattern rewritten into the numbering new_id (and downloaded into hp for the host-side layout code)
    int renumber_on_device(ogl::HostPattern &hp, const std::vector<ogl_label> &new_id);
    // the Hilbert-curve candidate of the numbering policy on the device: keys + radix sort, and the far-entry count
    int curve_on_device(ogl_label n, const double *centres, std::vector<ogl_label> &new_id);
    int curve_far_on_device(const ogl::HostPattern &hp, const std::vector<ogl_label> &new_id,
                            const std::vector<ogl_label> &old_of, int64_t &far);
    // renumbering (config `renumber`): pat.new_id on the device + a staging vector, so that host
    // vectors cross the boundary in the caller's cell order
    ogl::DevBuf<int32_t> d_new_id, d_old_of;
    ogl::DevBuf<double> d_perm_tmp;
    int pat_renumber_mode = -1;  // cfg.renumber / layout eligibility the pattern was built under
    bool pat_try_sell = false, pat_try_sym = false;
    ogl::DevBuf<double> d_flag;  // 2 doubles: cross-rank agreement on pattern rebuilds
    // host -> device / device -> host of one row vector, through the renumbering when there is one
    int upload_rows(double *dst, const double *src);
    int download_rows(double *dst, const double *src);
    // peer-put halo exchange (PeerHalo, kernels.hpp): agreed per sparsity pattern by all ranks
    struct PeerNeighbour {
        size_t block = 0;   // the neighbour's arena block (words from its arena start)
        int32_t n_neigh = 0, my_index = 0, n_halo = 0, my_seg = 0;  // its layout, this rank's place
    };
    bool peer_halo = false;
    size_t peer_block = 0;  // this solver's arena block
    size_t peer_block_words = 0;
    std::vector<PeerNeighbour> peer_nb;
    uint32_t halo_seq = 0;
    ogl::DevBuf<int32_t> d_boundary_chunk_ptr;  // ranges of boundary_rows per boundary chunk
    // the same ranges for EVERY chunk (HaloFused: the local SpMV kernel adds the non-local part itself) and the
    // send list grouped by the chunk of its rows (HaloPutFused: step_1x puts the halo values it has just formed)
    ogl::DevBuf<int32_t> d_chunk_bptr, d_chunk_sptr, d_send_pos;
    int32_t n_put_chunks = 0;
    ogl::PeerHalo cur_halo{};   // arguments of the SpMV whose halo values a producer kernel has already put
    ogl::HaloPutFused begin_halo_put();
    ogl::HaloFused halo_fused_args(const ogl::PeerHalo &ph) const;
    ogl::DevBuf<unsigned> d_ticket;             // last-workgroup ticket of k_pack_put_signal
    // a full batch of single-rank GKOCG turns captured as a hipGraph (run_krylov)
    hipGraphExec_t cg_graph = nullptr;
    uint64_t cg_graph_key = 0;  // hash of everything the captured launches bake in (launch_key.hpp)
    void drop_cg_graph();  // (every pattern / layout rebuild)
    int setup_peer_halo();
    // value_bytes: 8, or 4 for the mixed mode's halo (the receive blocks viewed as floats)
    ogl::PeerHalo peer_halo_args(uint32_t seq, size_t value_bytes) const;
    ogl::PeerHalo next_exchange(size_t value_bytes);  // the next number of halo_seq and its arguments
    void *peer_recv_block(uint32_t seq) const;        // this rank's receive block of exchange `seq`
    template <class T>
    T *peer_recv(uint32_t seq) const { return static_cast<T *>(peer_recv_block(seq)); }
    // a distributed product's halo before and after its local kernel, every transport but the fused peer-put
    // (solver_transport.cpp; T = double with HaloOwner, float with MixedHaloOwner)
    template <class T, class Owner>
    int halo_begin(const T *x, const Owner &own, ogl::PeerHalo &ph);
    template <class T, class Owner>
    int halo_end(int mode, const ogl::PeerHalo &ph, const T *nl_vals, T *y, const ogl::SpmvDotsOf<T> &dots, const Owner &own);
    // halo part
    std::vector<int32_t> boundary_rows, boundary_ptrs;
    ogl::DevBuf<int32_t> d_boundary_rows, d_boundary_ptrs, d_nl_cols, d_send_idxs;
    ogl::DevBuf<int32_t> d_boundary_chunks;  // chunks (of CHUNK_ROWS rows) that hold boundary rows
    int32_t n_boundary_chunks = 0;
    ogl::DevBuf<double> d_nl_vals, d_send, d_recv;
    std::vector<double> h_nl_vals;
    std::vector<int> neighbours, counts;

    // ---- vectors: "<field>_rhs", "<field>_solution" + Krylov work vectors ----
    ogl::DevBuf<double> d_x, d_b, d_r, d_p, d_q, d_w, d_inv_diag;
    ogl::DevBuf<double> d_p2;  // second p buffer of the 2-launch turn (k_cg_turn_sym)
    ogl::DevBuf<double> d_pring[ogl::P_RING_MAX - 2];  // further p buffers of the leader turn's ring (PRing, deferX)
    ogl::DevBuf<double> d_p_halo;  // multi-rank merged turn: old / new p at the halo columns
    ogl::DevBuf<double> d_bj_tmp0, d_bj_tmp1;  // block Jacobi through a permutation, staged apply: in / out in the caller's order
    ogl::DevBuf<double> d_v, d_s, d_t, d_y, d_z, d_rr;  // BiCGStab
    ogl::DevBuf<double> d_V, d_gm;                      // GMRES: Krylov bases, dense state
    ogl::DevBuf<float> d_Vf;  // the basis stored in fp32 (property basisPrecision single): sized in krylov_prepare by such a solve only
    // orthoMethod cgs | cgs2: (m + 1) x n_chunks partials of a round's dot products and its m + 1 coefficients; sized in
    // krylov_prepare, never for mgs (a solve on mgs leaves them as they are)
    ogl::DevBuf<double> d_gs_part, d_gs_h;
    ogl::DevBuf<double> d_isai_tmp;                     // ISAI(spd): W r before W^T
    ogl::DevBuf<double> d_fac_tmp[3];  // IC / ILU / IRILU: vectors in the caller's order, IRILU's iterates
    // Chebyshev: [0] the second iterate of the recurrence, [1] t = r - A z of the unfused step (held only while it runs)
    ogl::DevBuf<double> d_cheb_tmp[2];
    bool cheb_fused = false;  // this solver's applies run k_cheb_step_sym (prepare_apply: chebyshevFused on SpmvLayout::Sym)
    // Multigrid: generation of the hierarchy (per-round and per-level sizes are the only host round trips) and one V-cycle
    // (keyword aggregateCaching: generate_multigrid is a refresh -- the values under the aggregates P holds, no host round
    //  trip -- where P's record allows it, else the full generation)
    int generate_multigrid(ogl::PrecondData &P);
    int generate_multigrid_full(ogl::PrecondData &P, const ogl::MultigridPart::KeptFor &asking, int keep);
    int refresh_multigrid(ogl::PrecondData &P);
    void publish_multigrid(const ogl::MultigridPart &M);  // the read-only properties that describe a generated hierarchy
    int mg_caller_numbered_level0(ogl::PrecondData &P);  // a renumbered device copy: level 0's pattern in the caller's numbering
    void apply_multigrid(const double *in, double *out, const ogl::DevScalars *gate, double *dot_part);
    // the matrix a level really is: level 0 that keeps none of its own is the system matrix's CSR arrays (double; in single
    // precision such a level has no CSR matrix, and nothing that needs one -- the tail -- is given level 0)
    template <class T>
    ogl::MgCsrOf<T> mg_matrix(const ogl::MgLevel &L) const;
    // The cycle, one body for both operand types (instantiated for double and float in solver_mg.cpp).  What differs
    // between them at level 0 is in the overloads below it; every step counts its launches in `run`.
    template <class T>
    void mg_cycle(int level, const T *b, T *x, const ogl::MgWide &ends, ogl::MgRun &run, bool continued);
    template <class T>
    ogl::MgTailOf<T> mg_tail_table(int first, bool continued) const;
    // A x of a level: on its own CSR matrix, or (level 0 without one) on the in-loop layout, local part only
    void mg_product(const ogl::MgLevel &L, const double *x, double *y, ogl::MgRun &run);
    void mg_product(const ogl::MgLevel &L, const float *x, float *y, ogl::MgRun &run);
    // one sweep of level 0 on the in-loop layout, x_out = x + omega ((b - A x) / d) (out64: written there as doubles)
    void mg_layout_sweep(const ogl::MgLevel &L, const double *b, const double *x, double *x_out, double *out64, ogl::MgRun &run);
    void mg_layout_sweep(const ogl::MgLevel &L, const float *b, const float *x, float *x_out, double *out64, ogl::MgRun &run);
    // what the restriction of level 0 on the in-loop layout reads, left in the level's t; returns what it is
    ogl::MgRestrictFrom mg_layout_residual(const ogl::MgLevel &L, const double *b, const double *x, ogl::MgRun &run);
    ogl::MgRestrictFrom mg_layout_residual(const ogl::MgLevel &L, const float *b, const float *x, ogl::MgRun &run);
    int prepare_multigrid_apply();
    int mg_coarse_visits = 1;  // keyword coarseVisits as this solver's applies use it (prepare_multigrid_apply)
    int mg_sweeps = 2;         // keyword smootherSweeps, likewise: sweeps before and after the coarse correction
    double mg_scale = 1.0;     // keyword correctionScale, likewise: the factor on every prolongated correction
    // keyword cyclePrecision as this solver's applies use it: the cycle on binary32 operands
    bool mg_single = false;
    int prepare_multigrid_single();  // the levels' twin, the fine level's fp32 copy, the vectors; the overflow check
    // level 0's product in single precision with its epilogue (one launch)
    void mg_fine32(ogl::MxEpilogue epi, const float *x, const ogl::MgEpi &e, ogl::MgRun &run);
    int check_multigrid_keywords();
    int mg_tail_first = 0;  // first level the single-workgroup tail kernel takes in this solver's applies (mg_levels: none)
    bool precond_ready = false;        // a solve has set up precond_data (ogl_solver_apply_preconditioner)
    uint64_t precond_serial = 0, precond_pat = 0;  // ... the object's serial and this solver's pattern at that time
    bool precond_current() const;      // precond_data is still what the last solve set up, for this pattern
    // this solver's launch segments of the factor's level schedules ((first level, end level, thin) triples, property
    // iluThinRows), formed when the preconditioner is set up for a solve
    std::vector<int32_t> fac_seg_fwd, fac_seg_bwd;
    bool fac_isai_scratch = false;  // the last apply set up here ran triangularSolves isai (its scratch is held)
    ogl::DevBuf<double> d_part0, d_part1, d_part2;  // (part2: beta partials of the fused-finaliser turn)
    int64_t band_order_rows = 0;
    bool source_diag_valid = false;  // d_source's diagonal segment is the diagonal of d_vals (set by the coefficient update)
    int64_t csr_band_rows = 0;   // band of the device CSR arrays (csr_band), valid for pattern csr_band_pat
    uint64_t csr_band_pat = 0;
    int csr_band(int64_t *band);
    ogl::DevBuf<int32_t> d_band_order;  // band-aware workgroup order of the CSR-stream / compressed kernels (property spmvBandRows)
    ogl::DevBuf<double> d_part3, d_part4, d_part5;  // (the folded GKOBiCGStab turn: sum|s|, s.t, t.t)
    ogl::DevBuf<ogl::DevScalars> d_scal;
    ogl::DevBuf<double> d_history;
    ogl::DevScalars *h_scal = nullptr;  // pinned, 2 slots
    hipEvent_t poll_ev[2] = {nullptr, nullptr};
    unsigned long long *lead_box = nullptr;  // LeadBox of the leader finalisation (fine-grained, LEAD_BOX_WORDS words)
    // the held-z turn (k_cg_step2r1x): the chunks' tagged partials (fine-grained, 4 words per chunk) and what the census of
    // its resident grid said (0: not run yet, 1: all workgroups on the chip at once, -1: not -- the three-launch turn runs)
    unsigned long long *held_z_box = nullptr;
    size_t held_z_words = 0;
    int held_z_census = 0, held_z_census_grid = 0;
    unsigned *held_q_heads = nullptr;  // the queue heads phase S of the held-q turn draws from (HQ_HEAD_WORDS words)
    hipEvent_t chk_ev[2] = {nullptr, nullptr};  // brackets one evaluated criterion check per solve (time_for_res_norm_eval)
    bool x_resident = false, b_resident = false;
    ogl::PrecondData own_precond;              // regenerated-for-this-solve preconditioner
    const ogl::PrecondData *precond_data = nullptr;  // the one in use (own or the registry's)
    const double *precond = nullptr;  // scalar Jacobi: inverse diagonal (fused path); else nullptr

    // ---- per-field properties (common/common.C:75-146) ----
    std::map<std::string, double> props;

    // ---- last solve ----
    std::vector<double> history;
    double t_update_matrix_ms = 0;
    // profile_kernels
    std::vector<hipEvent_t> prof_ev;

    ~ogl_solver();

    int set_matrix(const ogl_ldu_view &ldu);
    int solve(const double *source, double *psi, ogl_perf *perf);
    int apply_resident(ogl_perf *perf);
    int upload_vec(ogl::DevBuf<double> &dst, const double *src);
    int ensure_vectors();
    int init_preconditioner();
    // generate_preconditioner dispatches on the kind; each generator: pattern-only part if the object does not hold it
    // for this pattern, then the values (generate_multigrid: above)
    int generate_preconditioner(ogl::PrecondData &P);
    // PrecondData::stride of a kind under this solver's keywords: what a stored object must match to be adopted
    int precond_stride(ogl::PrecondKind kind) const
    {
        if (kind == ogl::PrecondKind::BlockJacobi) return cfg.max_block_size;
        if (ogl::is_isai(kind)) return cfg.sparsity_power;
        return kind == ogl::PrecondKind::Chebyshev ? (int)keyword<ogl::ChebKeyword::chebyshevDegree>() : 0;
    }
    int generate_jacobi(ogl::PrecondData &P);
    int generate_inv_diag(ogl::DevBuf<double> &inv_diag);  // 1 / d of the device copy (scalar Jacobi, Chebyshev's w)
    int generate_chebyshev(ogl::PrecondData &P);
    int generate_block_jacobi(ogl::PrecondData &P, bool through_perm);
    int generate_isai(ogl::PrecondData &P, bool caller_numbering);
    int generate_factor(ogl::PrecondData &P);
    int prepare_apply();  // this solver's scratch and launch schedule for applies of precond_data
    void apply_factor(const double *in, double *out, const ogl::DevScalars *gate, double *dot_part);
    void apply_chebyshev(const double *in, double *out, const ogl::DevScalars *gate, double *dot_part);
    int check_factor_breakdown(int32_t word);
    // the preconditioner's breakdown word, where the kind in use has one: the address the final scalars take it from
    const int32_t *precond_breakdown_word() const;
    int check_chebyshev_breakdown(int32_t word);  // also reads the bounds in use back for the reports
    int check_chebyshev_keywords();  // chebyshevDegree, chebyshevEigRatio, chebyshevLambdaMax
    int check_factor_keywords();  // keywords triangularSolves and factorSweeps: validation, and IRILU + isai refused
    // out = M^-1 in for every kind (the Krylov loops fuse scalar Jacobi through `precond` instead); dot_part != nullptr:
    // also the per-chunk partials of sum_i in_i * out_i (CG's rho), out of the same kernel where the kind has one
    void apply_preconditioner(const double *in, double *out, const ogl::DevScalars *gate,
                              double *dot_part = nullptr);
    // prepacked: the kernel that produced x has put the halo values already (begin_halo_put)
    int dist_spmv(int mode, const double *x, const double *b, double *y, const ogl::SpmvDots &dots,
                  const ogl::DevScalars *gate, bool prepacked = false);
    // the local SpMV on layout l (the in-loop one: spmv_layout)
    void spmv_on(ogl::SpmvLayout l, int mode, const double *x, const double *b, double *y, const ogl::SpmvDots &dots,
                 const ogl::DevScalars *gate, const ogl::HaloFused &hf = ogl::HaloFused{});
    int finalize(int phase, ogl::FinArgs &a);
    template <class Args, class Launch>
    int split_finaliser(Args &a, double *sums, int n_sums, Launch launch);  // (solver_internal.hpp)
    int run_cg(ogl_perf *perf);
    int run_bicgstab(ogl_perf *perf);
    int run_krylov(ogl_perf *perf);
    // mixed precision (property mixedPrecision; solver_mixed.cpp): fp32 inner CG under an fp64 iterative refinement
    ogl::MixedPart mixed;
    int mixed_requested(bool *on);      // the keywords' validation and the refusals (OGL_ERR_INVALID / _UNSUPPORTED)
    // buffers, the scalars reset for a solve, the fp32 copy of the matrix current for this values epoch
    int mixed_storage(const ogl::DevCriterion &crit, double inner_rel_tol, int inner_max_iter);
    int fp32_bad_row(int64_t position, int64_t *row) const;  // the device row of a position in fp32_dev's value array
    int mixed_overflow(const ogl::MixedScalars &m);  // OGL_ERR_INVALID naming the row when a value overflowed binary32
    // q = A32 p: the local product, on several ranks between the halo's put (or pack + exchange) and its non-local part
    int mixed_spmv(const float *x, float *y, double *part, const ogl::MixedScalars *gate);
    // a finaliser of the mode with its sums all-reduced over the ranks (split_finaliser)
    int mixed_fin(int phase, ogl::MixedFinArgs &a);
    int run_mixed(ogl_perf *perf);
    // property orthoMethod (0 mgs | 1 cgs | 2 cgs2; GKOGMRES only, ignored elsewhere): its validation and the refusal on
    // several ranks (OGL_ERR_INVALID / _UNSUPPORTED)
    int ortho_requested(int *method);
    // property basisPrecision (0 double | 1 single; GKOGMRES only, ignored elsewhere): its validation and the refusal with mgs
    int basis_requested(bool *single);
    int spmv_f32(const float *x, float *y);
    // keyword guessProjection (solver_proj.cpp): x0 + sum_j alpha_j d_j over the stored steps of the
    // last solves in place of x0, then the same solve
    ogl::ProjPart proj;
    int proj_requested(int *K);   // the keyword's validation and the refusal on several ranks
    int proj_sync(int K);         // what clears the ring (guessProjectionReset, a change of K or of the pattern); the buffers
    int proj_credit_requested(int K, bool mixed_on, bool *credit);  // keyword guessProjectionCredit: validation, the refusal
    int proj_products_requested(bool *one_pass);                    // keyword guessProjectionProducts: validation
    int proj_pre_step(int K, bool credit, bool one_pass);  // before anything of the solve: x0 kept, the projection applied to d_x
    void proj_credit(hipStream_t st, ogl::DevScalars *s);  // after the scalars' reset: S0 into the criterion's state
    int proj_post_step(int rc, const ogl_perf *perf);  // after it: the step stored, the properties
    int set_guess_history(const double *vectors, int32_t k);
    int get_guess_history(double *out, int32_t capacity, int32_t *k);
    // run_krylov = plan -> prepare -> loop -> finish; one function per solver x turn shape (solver.cpp)
    struct KrylovRun;
    int krylov_plan(KrylovRun &k);
    int krylov_prepare(KrylovRun &k);
    int krylov_loop(KrylovRun &k);
    int krylov_enqueue(KrylovRun &k, int count);
    int krylov_finish(KrylovRun &k, ogl_perf *perf);
    int gmres_restart(KrylovRun &k, const ogl::DevScalars *gate);
    int gmres_update_x(KrylovRun &k, int cols, const ogl::DevScalars *gate);
    int turn_gmres(KrylovRun &k, int enq, int pe);
    int turn_gmres_f32_basis(KrylovRun &k, int it, int pe);
    int time_ortho_kernels(KrylovRun &k);  // (property orthoTimedLaunches: measurements only)
    int turn_cg_generic(KrylovRun &k, int enq, int pe);
    int turn_cg_generic_led(KrylovRun &k, int enq, int pe);
    int turn_cg_two_launch(KrylovRun &k, int enq, int pe);
    int turn_cg_three_launch(KrylovRun &k, int enq, int pe);
    int turn_cg_held_z(KrylovRun &k, int enq, int pe);
    int turn_cg_held_q(KrylovRun &k, int enq, int pe);
    int plan_held_z(KrylovRun &k);
    int turn_cg_merged(KrylovRun &k, int enq, int pe);
    int turn_cg_five_launch(KrylovRun &k, int enq, int pe);
    int turn_bicg_folded(KrylovRun &k, int enq, int pe);
    int turn_bicg(KrylovRun &k, int enq, int pe);
    int time_spmv(int repeats, double *avg_ms);
    ogl::DevHalo halo() const;
    // The input properties (properties.hpp): a read names its knob by identifier and takes the table's default; only a
    // knob of the computed kind takes its default from the call site, and only it may.
    double knob_value(ogl::Knob k, double dflt) const;
    template <ogl::Knob K>
    double knob() const
    {
        static_assert(ogl::knob_entry(K).dflt.kind != ogl::KnobKind::Computed, "a computed knob takes its default from the call site");
        return knob_value(K, ogl::knob_entry(K).dflt.value);
    }
    template <ogl::Knob K>
    double knob(double computed_default) const
    {
        static_assert(ogl::knob_entry(K).dflt.kind == ogl::KnobKind::Computed, "this knob's default stands in the table");
        return knob_value(K, computed_default);
    }
    template <ogl::Knob K>
    void set_knob(double v)  // (the effective value written back, or state)
    {
        static_assert(ogl::knob_entry(K).written_back || ogl::knob_entry(K).dflt.kind == ogl::KnobKind::State,
                      "the library writes only state and the knobs marked WRITTEN_BACK");
        props[ogl::knob_entry(K).name] = v;
    }
    int check_knob(ogl::Knob k) const;  // the current value against the table's domain: OGL_ERR_INVALID, one phrasing
    int check_entry(const ogl::KnobEntry &e) const;  // ... of any entry (check_knob; the Chebyshev keywords)
    template <ogl::ChebKeyword K>
    double keyword() const  // an input of preconditioner Chebyshev (properties.hpp, OGL_CHEB_KEYWORDS)
    {
        const auto it = props.find(ogl::knob_entry(K).name);
        return it == props.end() ? ogl::knob_entry(K).dflt.value : it->second;
    }
    // ogl_solver_set_matrix_like: the solver whose device copy of upper / lower this set_matrix may take (only during
    // that call), and what THIS solver's copy was uploaded from (host arrays + sampled checksum) for a later taker
    const ogl_solver *share_from = nullptr;
    const double *offdiag_upper = nullptr, *offdiag_lower = nullptr;
    uint64_t offdiag_sum = 0;
    bool offdiag_valid = false;
    // the addressing arrays of the last set_matrix (a sibling on the same arrays need not hash them again)
    const ogl_label *seen_lower_addr = nullptr, *seen_upper_addr = nullptr;
    ogl_label seen_faces = -1;
    struct SeenIface {  // (everything addressing_fingerprint mixes in per interface, by identity / value)
        const ogl_label *face_cells;
        ogl_label size, kind, neighb_proc, neighb_patch;
    };
    std::vector<SeenIface> seen_iface_cells;
    bool saw_addressing(const ogl_ldu_view &ldu) const;
    bool peer_safe_wait() const;
    double stream_above_bytes() const;
    double turn_extra_bytes() const;
    int32_t xcd_group() const;
    int32_t pat_xcd_group = 0;  // chosen per pattern (0 = the built-in group of 4 chunks)
};
