// kernels_spmv_sym.hip -- half-storage SpMV of banded symmetric patterns and the GKOCG turn kernels built on it
// (geometry, reduction tree and the -ffp-contract=off rule: device_common.hpp; the layout and its row walk -- planes,
// twins, gathers, the sum in ascending column order -- and the ladder over ND, FAST, STREAM: sym_walk.hpp)
#include <algorithm>

#include "device_common.hpp"
#include "resident_cg_turn.hpp"
#include "sym_walk.hpp"

namespace ogl {

namespace {

template <int MODE, int NDOT, int ND, bool FAST, bool STREAM>
__global__ __launch_bounds__(BLOCK) void k_spmv_sym(int n_rows, int n_chunks, SymOffsets off,
                                                    const uint8_t *__restrict__ mask,
                                                    const double *__restrict__ planes,
                                                    const double *__restrict__ x, const double *__restrict__ b,
                                                    double *__restrict__ y, const double *__restrict__ w,
                                                    double *__restrict__ dot_partials,
                                                    double *__restrict__ dot2_partials, const DevScalars *gate,
                                                    const int *__restrict__ block_order, HaloFused hf)
{
    __shared__ double slot[N_WAVES];
    __shared__ double ys[CHUNK_ROWS];
    if (gate && gate->stop) return;
    // banded patterns: the host's order puts the chunks of rows r and r +- d[ND-1] on one XCD (band_block_order)
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const RowPair rp = my_rows(chunk, n_rows);
    double2 xd;
    double2 acc = sym_rows<MODE, double, ND, FAST, STREAM>(chunk, rp, n_rows, off, mask, planes, x, b, xd);
    if (hf.chunk_bptr) halo_fused_add<MODE>(hf, chunk, acc.x, acc.y, ys);
    st2(y, rp, acc);
    if (NDOT >= 1) {
        const double2 vw = ld2(w, rp);
        double d = 0.0, d2 = 0.0;
        if (rp.n > 0) {
            d += vw.x * acc.x;
            d2 += acc.x * acc.x;
        }
        if (rp.n > 1) {
            d += vw.y * acc.y;
            d2 += acc.y * acc.y;
        }
        const double s = block_sum(d, slot);
        if (threadIdx.x == 0) dot_partials[chunk] = s;
        if (NDOT >= 2) {
            const double s2 = block_sum(d2, slot);
            if (threadIdx.x == 0) dot2_partials[chunk] = s2;
        }
    }
}

// The matrix work of the guess projection's pre-step (keyword guessProjectionProducts onePass; solver_proj.cpp, DESIGN.md
// section 7f) in one pass over the planes: r0 = b - A x0 and w_j = A d_j, j < k <= PROJ_MAX.  A thread loads its mask, its
// own planes and the twins of its lower entries once and keeps them; every vector then costs its gathers and one store --
// 33 N + 8 N (b) + 16 N (k + 1) bytes instead of 49 N (k + 1) + 8 N.  Gathers and sums are the functions k_spmv_sym runs
// (sym_walk.hpp), so r0 and every w_j have the bits of the k + 1 separate products.  The vectors go in batches of
// PROJ_BATCH: the gathers of a batch are in flight together, and the registers are the planes' 2 ND pairs plus the
// batch's (2 ND + 1) pairs whatever k is.  Under STREAM the once-read planes still pass the caches, once.
constexpr int PROJ_BATCH = 2;
template <int ND, bool FAST, bool STREAM>
__global__ __launch_bounds__(BLOCK) void k_proj_products_sym(int n_rows, int n_chunks, SymOffsets off,
                                                             const uint8_t *__restrict__ mask,
                                                             const double *__restrict__ planes,
                                                             const double *__restrict__ x0, const double *__restrict__ b,
                                                             double *__restrict__ r0, ProjProducts v,
                                                             const int *__restrict__ block_order)
{
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const RowPair rp = my_rows(chunk, n_rows);
    const unsigned mm = *reinterpret_cast<const unsigned short *>(mask + rp.row);
    const unsigned m0 = mm & 0xffu, m1 = mm >> 8;
    double2 up[ND], lo[ND];
    sym_own_planes<double, ND, FAST, STREAM>(up, chunk, planes);
    {
        double2 xl[ND], xu[ND];
        const double2 acc = ld2(b, rp), xd = ld2(x0, rp);
        sym_twin_planes<double, ND, FAST, STREAM>(lo, up, rp.row, off, planes);
        sym_gather<double, ND, FAST>(xl, xu, xd, rp.row, n_rows, off, x0);
        st2(r0, rp, sym_sum<SPMV_RESIDUAL, double, ND>(m0, m1, up, lo, xd, xl, xu, acc));
    }
#pragma unroll 1
    for (int j0 = 0; j0 < v.k; j0 += PROJ_BATCH) {
        double2 dl[PROJ_BATCH][ND], du[PROJ_BATCH][ND], dd[PROJ_BATCH];
#pragma unroll
        for (int e = 0; e < PROJ_BATCH; ++e) {  // (past the last vector: the last one once more, loaded and not used)
            const double *__restrict__ d = v.in[min(j0 + e, v.k - 1)];
            dd[e] = ld2(d, rp);
            sym_gather<double, ND, FAST>(dl[e], du[e], dd[e], rp.row, n_rows, off, d);
        }
#pragma unroll
        for (int e = 0; e < PROJ_BATCH; ++e) {
            if (j0 + e >= v.k) break;
            double2 zero;
            zero.x = zero.y = 0.0;
            st2(v.W + (size_t)(j0 + e) * v.ld, rp, sym_sum<SPMV_PLAIN, double, ND>(m0, m1, up, lo, dd[e], dl[e], du[e], zero));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Small systems on half storage, two launches per GKOCG turn: step_1x_fin and the SpMV in one kernel.  The SpMV
// needs p_new = z + (rho/rho') p at the columns of its rows, which other workgroups own -- but p_new is an
// elementwise function of z (which step_2r_fin leaves behind for this; r itself without a preconditioner) and the
// old p, so every workgroup recomputes it for the columns it gathers (same expression, same rounding:
// -ffp-contract=off) instead of waiting for a kernel boundary.  The new p of the
// own rows goes to the other of two p buffers (neighbours still read the old one).  Everything else -- check of
// the previous turn, pending x update, row sums in ascending column order, partial of p.q -- is what
// k_cg_step1x_fin followed by k_spmv_sym<SPMV_PLAIN, 1> does, bit for bit.
//   turn = [this kernel] -> k_cg_step2r_fin
// ------------------------------------------------------------------------------------------
// what a thread of the merged kernels holds of its two rows: [0] p, [1] z at the rows and at the gathered columns,
// own planes (diagonal, upper entries) and the twins of the lower entries
template <int ND>
struct TurnSymRegs {
    double2 vd[2], vl[2][ND], vu[2][ND], up[ND], lo[ND];
};
// The walk's loads (sym_walk.hpp), the vectors first, then the matrix; none waits for the mask -- a small system is all latency
template <int ND, bool FAST, bool STREAM>
__device__ __forceinline__ void turn_sym_load(TurnSymRegs<ND> &R, int chunk, const RowPair &rp, int n_rows,
                                              const SymOffsets &off, const double *__restrict__ planes,
                                              const double *__restrict__ p_in, const double *__restrict__ z)
{
    R.vd[0] = ld2(p_in, rp);
    sym_gather<double, ND, FAST>(R.vl[0], R.vu[0], R.vd[0], rp.row, n_rows, off, p_in);
    R.vd[1] = ld2(z, rp);
    sym_gather<double, ND, FAST>(R.vl[1], R.vu[1], R.vd[1], rp.row, n_rows, off, z);
    sym_own_planes<double, ND, FAST, STREAM>(R.up, chunk, planes);
    sym_twin_planes<double, ND, FAST, STREAM>(R.lo, R.up, rp.row, off, planes);
}
// p_new = z + tmp p for the own rows (-> xd) and for every gathered column, then the walk's two row sums
template <int ND>
__device__ __forceinline__ double2 turn_sym_rows(const TurnSymRegs<ND> &R, unsigned m0, unsigned m1, double tmp,
                                                 double2 &xd)
{
    double2 xl[ND], xu[ND];
    xd.x = R.vd[1].x + tmp * R.vd[0].x;
    xd.y = R.vd[1].y + tmp * R.vd[0].y;
#pragma unroll
    for (int j = 1; j < ND; ++j) {
        xl[j].x = R.vl[1][j].x + tmp * R.vl[0][j].x;
        xl[j].y = R.vl[1][j].y + tmp * R.vl[0][j].y;
        xu[j].x = R.vu[1][j].x + tmp * R.vu[0][j].x;
        xu[j].y = R.vu[1][j].y + tmp * R.vu[0][j].y;
    }
    double2 acc;
    acc.x = acc.y = 0.0;
    return sym_sum<SPMV_PLAIN, double, ND>(m0, m1, R.up, R.lo, xd, xl, xu, acc);
}

// LEAD (more than FUSED_FIN_MAX_CHUNKS chunks): the first 32 workgroups of the launch are the finaliser's wavefronts, every
// workgroup fetches their sums from the mailbox (leader finalisation, device_common.hpp; k_cg_step1x_fin<true>)
template <int ND, bool FAST, bool LEAD>
__global__ __launch_bounds__(BLOCK) void k_cg_turn_sym(int n_rows, int n_chunks, SymOffsets off,
                                                       const uint8_t *__restrict__ mask,
                                                       const double *__restrict__ planes,
                                                       const double *__restrict__ p_in, double *__restrict__ p_out,
                                                       double *__restrict__ x, const double *__restrict__ z,
                                                       double *__restrict__ q,
                                                       double *__restrict__ part_beta, const DevScalars *sin,
                                                       DevScalars *sout, const double *__restrict__ part_rho,
                                                       const double *__restrict__ part_norm, int n_part,
                                                       double *history, int first,
                                                       const int *__restrict__ block_order, LeadBox lbox)
{
    __shared__ double red[2 * FIN_WAVES];
    __shared__ double sh[4];
    __shared__ int sh_stop;
    __shared__ double slot[N_WAVES];
    __shared__ double lead_words[LEAD ? LEAD_BOX_WORDS / 2 : 1];
    __shared__ double lead_stage[LEAD ? LEAD_STAGE : 1];
    __shared__ int lead_timed_out;
    const uint32_t seq = LEAD ? sin->launch_seq : 0u;
    if (LEAD) lead_leaders<2>(lbox, seq, part_rho, part_norm, nullptr, n_part, lead_stage);  // (by launch position, not by chunk)
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const bool lead = chunk == 0;  // the workgroup that stores the scalars and the history entry
    // scalars field by field (k_cg_step1x_fin), and every load of the kernel asked for before the first wait
    const int stopped = sin->stop;
    const double s_rho = sin->rho, s_beta = sin->beta, s_nf = sin->norm_factor, s_init = sin->init_res;
    const int s_iter = sin->iter, s_evals = sin->n_evals;
    const CritVals crit = load_criterion(sin->crit);
    if (lead && threadIdx.x < sizeof(DevScalars) / 8)
        reinterpret_cast<unsigned long long *>(sout)[threadIdx.x] =
            reinterpret_cast<const unsigned long long *>(sin)[threadIdx.x];
    const RowPair rp = my_rows(chunk, n_rows);
    const unsigned mm = *reinterpret_cast<const unsigned short *>(mask + rp.row);
    const unsigned m0 = mm & 0xffu, m1 = mm >> 8;
    double pv[2][FIN_VT];
    if (!LEAD) load_partials_as_finaliser<2>(part_rho, part_norm, n_part, pv);
    double2 vx = ld2(x, rp);
    TurnSymRegs<ND> R;
    turn_sym_load<ND, FAST, false>(R, chunk, rp, n_rows, off, planes, p_in, z);
    if (stopped) return;  // (the solve has ended: the lead workgroup has handed the scalars on)
    double v[2] = {0.0, 0.0};
    if (LEAD) {
        if (!lead_wait(lbox, 4 * FIN_WAVES, seq, lead_words, &lead_timed_out)) {
            if (threadIdx.x == 0) sout->comm_error = sout->stop = 1;
            return;
        }
        if (threadIdx.x == 0) {
            v[0] = lead_total(lead_words, 0);
            v[1] = lead_total(lead_words, 1);
        }
    } else {
        reduce_partials_as_finaliser<2>(pv, n_part, red, v);
    }
    if (threadIdx.x == 0) {
        // FIN_CG_CHECK: swap(prev_rho, rho) of the previous turn, then the criterion
        const double prev_rho = s_rho, rho = v[0];
        const Verdict cv = criterion_verdict(crit, s_iter, s_evals, s_init, s_nf, v[1], lead ? history : nullptr);
        sh[0] = s_beta;
        sh[1] = prev_rho;
        sh[2] = rho;
        sh_stop = cv.stop;
        if (lead) {
            sout->prev_rho = prev_rho;
            sout->rho = rho;
            sout->x_pending = 0;
            store_verdict(sout, cv);
            if (LEAD) sout->launch_seq = seq + 1;
        }
    }
    __syncthreads();
    const double beta = sh[0], prev = sh[1], rho = sh[2];
    const int stop = sh_stop;
    if (!first && beta != 0.0) {  // x += t_j p of the turn this check closed
        const double t = prev / beta;
        vx.x += t * R.vd[0].x;
        vx.y += t * R.vd[0].y;
        st2(x, rp, vx);
    }
    if (stop) return;
    const double tmp = (prev == 0.0) ? 0.0 : rho / prev;
    double2 xd;
    const double2 acc = turn_sym_rows<ND>(R, m0, m1, tmp, xd);
    st2(p_out, rp, xd);
    st2(q, rp, acc);
    double d = 0.0;
    if (rp.n > 0) d += xd.x * acc.x;
    if (rp.n > 1) d += xd.y * acc.y;
    const double sd = block_sum(d, slot);
    if (threadIdx.x == 0) part_beta[chunk] = sd;
}

// The same merge for systems of any size, between the single-workgroup finalisers of the five-launch turn (which
// becomes four): the scalars are read where k_cg_step1x reads them, the pending x update included.  Per turn the
// vectors cost 8 N bytes less than step_1x + SpMV + step_2r (p is read once, z written once and read once instead of
// r and 1/d read twice), and one kernel boundary goes.
// HALO (several ranks, peer-put transport): the neighbours' step_2r has put z of the halo columns; a workgroup whose
// chunk holds boundary rows waits for it, forms p_new at those columns from the old halo p it keeps (ph_in -> ph_out)
// and continues its boundary rows over their non-local entries -- no put and no wait for a put of THIS launch here.
template <int ND, bool FAST, bool STREAM, bool HALO>
__global__ __launch_bounds__(BLOCK) void k_cg_turn_sym_big(int n_rows, int n_chunks, SymOffsets off,
                                                           const uint8_t *__restrict__ mask,
                                                           const double *__restrict__ planes,
                                                           const double *__restrict__ p_in,
                                                           double *__restrict__ p_out, double *__restrict__ x,
                                                           const double *__restrict__ z, double *__restrict__ q,
                                                           double *__restrict__ part_beta, const DevScalars *s,
                                                           const int *__restrict__ block_order, HaloFused hf,
                                                           const double *__restrict__ ph_in,
                                                           double *__restrict__ ph_out)
{
    __shared__ double slot[N_WAVES];
    const int stop = s->stop;
    const bool pending = s->x_pending != 0;
    if (stop && !pending) return;
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const RowPair rp = my_rows(chunk, n_rows);
    if (stop) {  // the solve has ended with an update still to apply: that only
        const double beta = s->beta;
        if (beta != 0.0) {
            const double t = s->prev_rho / beta;
            const double2 vp = ld2(p_in, rp);
            double2 vx = ld2_stream(x, rp);
            vx.x += t * vp.x;
            vx.y += t * vp.y;
            st2_stream(x, rp, vx);
        }
        return;
    }
    const unsigned mm = *reinterpret_cast<const unsigned short *>(mask + rp.row);
    const unsigned m0 = mm & 0xffu, m1 = mm >> 8;
    TurnSymRegs<ND> R;
    turn_sym_load<ND, FAST, STREAM>(R, chunk, rp, n_rows, off, planes, p_in, z);
    if (pending) {
        const double beta = s->beta;
        if (beta != 0.0) {
            const double t = s->prev_rho / beta;
            double2 vx = ld2_stream(x, rp);  // x is touched once per turn
            vx.x += t * R.vd[0].x;
            vx.y += t * R.vd[0].y;
            st2_stream(x, rp, vx);
        }
    }
    const double rho = s->rho, prev = s->prev_rho;
    const double tmp = (prev == 0.0) ? 0.0 : rho / prev;
    double2 xd;
    double2 acc = turn_sym_rows<ND>(R, m0, m1, tmp, xd);
    st2(p_out, rp, xd);
    if (HALO) {
        __shared__ double ys[CHUNK_ROWS];
        if (hf.chunk_bptr) halo_fused_add<SPMV_PLAIN, true>(hf, chunk, acc.x, acc.y, ys, tmp, ph_in, ph_out);
    }
    st2(q, rp, acc);
    double d = 0.0;
    if (rp.n > 0) d += xd.x * acc.x;
    if (rp.n > 1) d += xd.y * acc.y;
    const double sd = block_sum(d, slot);
    if (threadIdx.x == 0) part_beta[chunk] = sd;
}

// ------------------------------------------------------------------------------------------
// The held-q turn (streamed single-rank GKOCG on half storage, scalar Jacobi or none): the SpMV in front of the held-z
// turn (kernels_krylov.hip, k_cg_step2r1x; the body both kernels run: resident_cg_turn.hpp), ONE launch per turn.
// q = A p, which the SpMV would write and step_2r read back (16 N bytes per turn), stays where z will be: in registers
// (R slots per workgroup) and LDS (L slots); only the grid-wide sum beta = p.q stands between the two.
//   turn = [ S: q = A p, held | beta | R: r' = r - t q, z in q's place | rho, sum |r'| | H: check, x, p_new ]
//   slot i of workgroup w holds the chunk at POSITION w + i G of the SpMV's launch order (the band order with its -1
//   holes, or xcd_chunk): with G a multiple of 8 a chunk's far neighbours sit on its own XCD, as in the stand-alone SpMV.
//   Any other G computes the same bits but sends them to other L2s; the host turns the kernel on by default only where
//   G % 8 == 0 (plan_held_z).
//   The same map in all three phases; holes and positions past the end own nothing.  That is the STATIC map; by default
//   only a workgroup's first slots follow it and the others are drawn (below, at HeldQSrc), from HQ_R + L = 22 slots.
//   phase S: sym_rows on p; the chunk's partial of p.q goes out as a tagged word (6 words per chunk: beta | rho | sum|r'|),
//     tag `seq`.  Sixteen workgroups poll those partials in the finaliser's order (lead_wave_sums_tagged: the bits of
//     lead_leaders<1> over the stand-alone SpMV's partials) and publish where the body's first wait looks.
//   phases R, the sums, H: the shared body, with q from the slot.  With K = 0, H overwrites p in place: beta is complete
//     only after every workgroup has finished S, and nobody passes the first wait before.
// A stopped solve returns before any poll; every spin is bounded by lead.timeout_ticks and ends the solve with comm_error.
// ------------------------------------------------------------------------------------------
// The draw (HeldQ, kernels.hpp; S = static_slots < HQ_STATIC): a static map cannot level workgroups whose rates differ, so
// only slot i < S of workgroup w holds position w + i G; the positions from S G on form eight queues -- position p is in
// queue p % 8, in launch order -- and workgroup w < drawers takes the next of queue w % 8 for each further slot: one
// returning atomic add of thread 0 on the queue's head, asked for one slot AHEAD, in front of the loads of the slot at
// work, and read by the workgroup behind the barrier block_sum has anyway (a draw costs a trip to memory: it must not
// stand in front of a slot's loads).  w % 8 is the XCD the workgroup runs on -- the assumption xcd_chunk makes, for speed
// only.  A drawn slot's position stays in LDS (drawn[]): the same map in all three phases.
//   Every position is computed, by exactly one workgroup: a ticket below the queue's length belongs to whoever drew it,
//   and a workgroup asks only while it has a free slot, so it computes what it draws.  A workgroup stops asking when its
//   R + L slots are full or its ticket is past the queue's end.  If one of the queue's workgroups stopped for the second
//   reason, every ticket below the length was drawn before; if all of them stopped for the first, they drew
//   drawers_of_the_queue * (R + L - S) tickets, and the host admits the draw only where that is >= the queue's length
//   (plan_held_z; else the static map runs).  Nobody waits for anybody's draw: phase S ends as it did.
//   The heads: two sets of eight, picked by the parity of the solve's held-q launches.  Workgroup 0 zeroes the OTHER set,
//   whose last users left at the kernel boundary before this launch and whose next come after this launch's end.  Zeroing
//   the set in use inside the launch that uses it would be wrong at any point: a workgroup that owns nothing polls for
//   nothing it must wait for and may still draw after workgroup 0 has passed both waits.
// the held-q turn's slots: positions of the SpMV's launch order with their holes; q of a chunk is in its slot; 6 tagged
// words per chunk (beta | rho | sum|r'|)
// DRAW false: the static map alone, and nothing of the draw in the code
template <bool DRAW>
struct HeldQSrc {
    static constexpr bool Q_HELD = true;
    static constexpr int STRIDE = 6, WORD = 2;
    int G, n_pos, n_partials;
    const int *__restrict__ block_order;
    int S;             // slots below S are static
    const int *drawn;  // LDS: the position of slot i >= S, -1 where it drew none
    __device__ __forceinline__ int chunk_at(int pos) const  // -1: a hole of the order, a position past its end, none
    {
        if (pos < 0 || pos >= n_pos) return -1;
        const int c = block_order ? block_order[pos] : xcd_chunk(pos);
        return c < n_partials ? c : -1;
    }
    __device__ __forceinline__ int chunk_of(int i) const
    {
        if constexpr (!DRAW) return chunk_at((int)blockIdx.x + i * G);
        return chunk_at(i < S ? (int)blockIdx.x + i * G : __builtin_amdgcn_readfirstlane(drawn[i]));
    }
    __device__ __forceinline__ int chunk_of_rolled(int i) const  // (resident_cg_turn.hpp, turn_chunk_rolled)
    {
        if constexpr (!DRAW) return chunk_at((int)blockIdx.x + i * G);
        return chunk_at(i < S ? (int)blockIdx.x + i * G : drawn[i]);
    }
};
template <int R, int L, int B, int K, int ND, bool FAST, bool DRAW>
__global__ __launch_bounds__(BLOCK, B) void k_cg_turn_held_q(int n, int n_chunks, int n_pos, SymOffsets off,
                                                             const uint8_t *__restrict__ mask,
                                                             const double *__restrict__ planes,
                                                             const int *__restrict__ block_order, double *__restrict__ r,
                                                             const double *__restrict__ inv_diag, double *p, double *p_out,
                                                             double *__restrict__ x, DevScalars *s,
                                                             unsigned long long *tagged, double *history, LeadBox lead,
                                                             const double *p_pend, int ring_phase, int early_slots,
                                                             int static_slots, int drawers, unsigned *heads, int parity)
{
    __shared__ double zl[L > 0 ? L * CHUNK_ROWS : 1];
    __shared__ TurnLds lds;
    __shared__ int drawn[DRAW ? R + L : 1];
    using Src = HeldQSrc<DRAW>;
    const TurnScalars ts = turn_prelude<K>(s, ring_phase);
    const TurnArgs a{n, r, inv_diag, p, p_out, x, s, tagged, history, lead, p_pend, early_slots};
    const int G = gridDim.x, w = blockIdx.x;
    const int S = DRAW ? static_slots : R + L;
    const Src src{G, n_pos, n_chunks, block_order, S, drawn};
    if (ts.stopped) return;  // (every workgroup sees the same flag: nobody polls, nobody writes)
    unsigned *const head = heads + (size_t)(parity * N_XCD + w % N_XCD) * HQ_HEAD_STRIDE;
    const int q0 = S * G + ((w % N_XCD) - (S * G) % N_XCD + N_XCD) % N_XCD;  // the queue's first position
    auto ask = [&]() { return __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto position = [&](unsigned ticket) {
        const long long pos = q0 + (long long)N_XCD * ticket;
        return pos < n_pos ? (int)pos : -1;
    };
    bool more = DRAW && w < drawers;  // (workgroup-uniform) the queue has not ended for this workgroup
    if constexpr (DRAW) {
        if (threadIdx.x < R + L) drawn[threadIdx.x] = -1;
        if (w == 0 && threadIdx.x < N_XCD) heads[(size_t)((parity ^ 1) * N_XCD + threadIdx.x) * HQ_HEAD_STRIDE] = 0u;
        if (more && S == 0 && threadIdx.x == 0) drawn[0] = position(ask());  // (the one draw nothing can hide)
        __syncthreads();
        if (more && S == 0) more = __builtin_amdgcn_readfirstlane(drawn[0]) >= 0;
    }
    // phase S: q = A p of every slot's chunk, kept; the partials of p.q
    TurnSlots<R, L> z;
    z.zl = zl;
#pragma unroll
    for (int i = 0; i < R + L; ++i) {
        const bool ahead = DRAW && more && i + 1 >= S && i + 1 < R + L;  // (workgroup-uniform) slot i + 1 draws
        unsigned ticket = 0;
        if (ahead && threadIdx.x == 0) ticket = ask();
        const int chunk = src.chunk_of(i);
        if (chunk < 0) {  // (workgroup-uniform; no break: the loop must unroll, see TurnSlots)
            if (ahead) {  // (a hole of the order: no block_sum to stand behind)
                if (threadIdx.x == 0) drawn[i + 1] = position(ticket);
                __syncthreads();
                more = __builtin_amdgcn_readfirstlane(drawn[i + 1]) >= 0;
            }
            continue;
        }
        const RowPair rp = my_rows(chunk, n);
        double2 xd;
        double2 vq = sym_rows<SPMV_PLAIN, double, ND, FAST, true>(chunk, rp, n, off, mask, planes, p, nullptr, xd);
        if (rp.n < 2) vq.y = 0.0;  // (rows past the end: what ld2_stream(q) gives the two-launch turn)
        if (rp.n < 1) vq.x = 0.0;
        z.put(i, vq);
        double d = 0.0;
        if (rp.n > 0) d += xd.x * vq.x;
        if (rp.n > 1) d += xd.y * vq.y;
        if (ahead && threadIdx.x == 0) drawn[i + 1] = position(ticket);
        const double sd = block_sum(d, lds.slot);
        if (ahead) more = __builtin_amdgcn_readfirstlane(drawn[i + 1]) >= 0;
        if (threadIdx.x == 0) put_tagged(tagged + Src::STRIDE * (size_t)chunk, ts.seq, sd);
    }
    // beta: sixteen workgroups -- behind the 2 x 16 of the later sums where the grid has them -- are the finaliser's wavefronts
    const int lead0 = G >= 3 * FIN_WAVES ? 2 * FIN_WAVES : 0;
    if (w >= lead0 && w < lead0 + FIN_WAVES)
        lead_wave_sums_tagged(lead, ts.seq, tagged, Src::STRIDE, n_chunks, w - lead0, 0);
    TurnFront<Src::Q_HELD> f;
    turn_ask_first(src, a, f);
    double beta;
    if (!turn_await_beta(a, ts, lds, beta)) return;
    resident_cg_turn<R, L, K>(src, a, ts, lds, z, f, beta);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void launch_spmv_sym(hipStream_t st, const DevSym &A, int mode, const double *x, const double *b, double *y,
                     const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto stream) {
        auto go = [&](auto m, auto ndot) {
            hipLaunchKernelGGL((k_spmv_sym<decltype(m)::value, decltype(ndot)::value, decltype(nd)::value,
                                           decltype(fast)::value, decltype(stream)::value>),
                               grid, block, 0, st, A.n_rows, nc, off, A.mask, A.planes, x, b, y, dots.with, dots.part,
                               dots.part_yy, gate, A.block_order, hf);
        };
        using Plain = std::integral_constant<int, SPMV_PLAIN>;
        if (mode == SPMV_RESIDUAL)
            go(std::integral_constant<int, SPMV_RESIDUAL>{}, std::integral_constant<int, 0>{});
        else if (dots.part && dots.part_yy)
            go(Plain{}, std::integral_constant<int, 2>{});
        else if (dots.part)
            go(Plain{}, std::integral_constant<int, 1>{});
        else
            go(Plain{}, std::integral_constant<int, 0>{});
    });
}

void launch_proj_products_sym(hipStream_t st, const DevSym &A, const double *x0, const double *b, double *r0,
                              const ProjProducts &v)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto stream) {
        hipLaunchKernelGGL((k_proj_products_sym<decltype(nd)::value, decltype(fast)::value, decltype(stream)::value>), grid,
                           block, 0, st, A.n_rows, nc, off, A.mask, A.planes, x0, b, r0, v, A.block_order);
    });
}

void launch_cg_turn_sym(hipStream_t st, const DevSym &A, const double *p_in, double *p_out, double *x, const double *z,
                        double *q, double *part_beta, const DevScalars *sin, DevScalars *sout,
                        const double *part_rho, const double *part_norm, double *history, int first, const LeadBox &lead)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    const bool led = lead.box && nc >= 3 * FIN_WAVES;
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto) {
        auto go = [&](auto is_led, const LeadBox &box) {
            hipLaunchKernelGGL((k_cg_turn_sym<decltype(nd)::value, decltype(fast)::value, decltype(is_led)::value>), grid,
                               block, 0, st, A.n_rows, nc, off, A.mask, A.planes, p_in, p_out, x, z, q, part_beta, sin, sout,
                               part_rho, part_norm, nc, history, first, A.block_order, box);
        };
        if (led)
            go(std::true_type{}, lead);
        else
            go(std::false_type{}, LeadBox{});
    });
}

void launch_cg_turn_sym_big(hipStream_t st, const DevSym &A, const double *p_in, double *p_out, double *x,
                            const double *z, double *q, double *part_beta, const DevScalars *s,
                            const HaloFused &hf, const double *p_halo_in, double *p_halo_out)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto stream) {
        auto go = [&](auto halo, const HaloFused &h, const double *ph_in, double *ph_out) {
            hipLaunchKernelGGL((k_cg_turn_sym_big<decltype(nd)::value, decltype(fast)::value, decltype(stream)::value,
                                                  decltype(halo)::value>),
                               grid, block, 0, st, A.n_rows, nc, off, A.mask, A.planes, p_in, p_out, x, z, q, part_beta, s,
                               A.block_order, h, ph_in, ph_out);
        };
        if (hf.chunk_bptr)
            go(std::true_type{}, hf, p_halo_in, p_halo_out);
        else
            go(std::false_type{}, HaloFused{}, nullptr, nullptr);
    });
}

// The held-q turn: ND as launch_spmv_sym has them, FAST both, the streaming loads only, p in place or two buffers
// -- and each of them twice: the static map on the held-z turn's 11 + 9 slots, the draw on 13 + 9
#define OGL_HELD_Q(K, ND, FAST, DRAW) k_cg_turn_held_q<DRAW ? HQ_R : HZ_R, HZ_L, HZ_B, K, ND, FAST, DRAW>
#define OGL_HELD_Q_EACH(DO) \
    DO(0, 2, false) DO(0, 2, true) DO(0, 3, false) DO(0, 3, true) DO(0, 4, false) DO(0, 4, true) \
    DO(2, 2, false) DO(2, 2, true) DO(2, 3, false) DO(2, 3, true) DO(2, 4, false) DO(2, 4, true)
int held_q_positions(const DevSym &A)
{
    return A.block_order ? A.n_blocks : xcd_grid((int)n_chunks(A.n_rows));
}

int held_q_occupancy(int *per_cu, size_t *lds_bytes)
{
    *per_cu = HZ_B;
    *lds_bytes = 0;
#define OGL_HELD_Q_ASK_ONE(K, ND, FAST, DRAW)                                                                            \
    {                                                                                                                    \
        int o = 0;                                                                                                       \
        hipFuncAttributes fa;                                                                                            \
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, OGL_HELD_Q(K, ND, FAST, DRAW), BLOCK, 0) != hipSuccess ||   \
            hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(OGL_HELD_Q(K, ND, FAST, DRAW))) != hipSuccess)      \
            return 1;                                                                                                    \
        *per_cu = std::min(*per_cu, o);                                                                                  \
        *lds_bytes = std::max(*lds_bytes, (size_t)fa.sharedSizeBytes);                                                   \
    }
#define OGL_HELD_Q_ASK(K, ND, FAST) OGL_HELD_Q_ASK_ONE(K, ND, FAST, false) OGL_HELD_Q_ASK_ONE(K, ND, FAST, true)
    OGL_HELD_Q_EACH(OGL_HELD_Q_ASK)
#undef OGL_HELD_Q_ASK
#undef OGL_HELD_Q_ASK_ONE
    return 0;
}

void launch_cg_turn_held_q(hipStream_t st, const DevSym &A, double *r, const double *inv_diag, double *p, double *p_out,
                           double *x, DevScalars *s, double *history, const LeadBox &lead, const PRing &ring,
                           const HeldZ &hz, const HeldQ &hq)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(hz.grid), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto) {
        auto go = [&](auto k, auto draw) {
            constexpr int K = decltype(k)::value;
            hipLaunchKernelGGL((OGL_HELD_Q(K, decltype(nd)::value, decltype(fast)::value, decltype(draw)::value)), grid, block,
                               0, st, A.n_rows, nc, hq.n_pos, off, A.mask, A.planes, A.block_order, r, inv_diag, p,
                               K == 2 ? p_out : p, x, s, hz.tagged, history, lead,
                               K == 2 ? (const double *)ring.b[1] : nullptr, K == 2 ? ring.phase : 0, hz.early_slots,
                               hq.static_slots, hq.drawers, hq.heads, hq.parity);
        };
        auto with_k = [&](auto k) {
            if (hq.static_slots < HQ_STATIC)
                go(k, std::true_type{});
            else
                go(k, std::false_type{});
        };
        if (ring.k == 2)
            with_k(std::integral_constant<int, 2>{});
        else
            with_k(std::integral_constant<int, 0>{});
    });
}
#undef OGL_HELD_Q_EACH
#undef OGL_HELD_Q

}  // namespace ogl
