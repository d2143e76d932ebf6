// resident_cg_turn.hpp -- the body of the resident GKOCG turn, shared by its two kernels (device only):
//   k_cg_step2r1x    (kernels_krylov.hip,   held-z: q comes from memory, the SpMV is a launch of its own)
//   k_cg_turn_held_q (kernels_spmv_sym.hip, held-q: the half-storage SpMV runs in front as phase S, q stays in the slots)
// Both must leave the same state bit for bit (tests/test_gpu_held_q.py); what differs between them is a `Src` type:
//   chunk_of(i)     the chunk of slot i of this workgroup, -1 where the slot owns nothing -- the same map in every phase
//   Q_HELD, q       where q of a slot's chunk is: in the slot itself, or in global memory (prefetched with r and 1/d)
//   STRIDE, WORD    the tagged box: STRIDE words per chunk, the partial of rho at WORD, of sum|r'| at WORD + 2.  The two
//                   layouts stay apart because a mixed solve runs both kernels on one box (plan_held_z)
//   n_partials      chunks of the system (what the finaliser's tree sums over)
// A kernel reads the scalars (turn_prelude), puts the sums of beta into the mailbox its own way, asks for the first rows
// (turn_ask_first), waits for beta (turn_await_beta) and runs resident_cg_turn: phase R (step_2r), the 2 x 16 leader sums,
// phase H (the head) -- the protocol is told at k_cg_step2r1x.  What must hold in here:
//   * the scalars stay in ONE slot: every workgroup has read every field it needs (turn_prelude, at the kernel's top)
//     before it publishes its first partial, and workgroup 0 writes only after it has seen the sums of ALL partials;
//   * the loops over the slots unroll fully, with `continue`, never `break`: the slots are indexed at compile time;
//   * a stopped solve returns before any poll; every spin is bounded by lead.timeout_ticks and ends the solve with
//     comm_error.
#pragma once
#include "device_common.hpp"

namespace ogl {

namespace {

constexpr int TURN_AHEAD = 2;  // chunks whose rows are in flight ahead of the one at work (phase R)

// what both kernels read from *s, field by field (criterion_verdict's comment, device_common.hpp), and the head's place
// in the ring of p buffers (K == 2: ring_phase = PRing::phase; the whole ring would cost 16 SGPRs)
struct TurnScalars {
    uint32_t seq;
    int stopped;
    double rho, norm_factor, init_res;
    int phase;         // ring position of the head in here
    bool defers;       // it leaves its term of x pending
    unsigned pending;  // defer_valid as it comes in
    double t1;         // t_ring[1]
    int iter, n_evals;
    CritVals crit;
};
template <int K>
__device__ __forceinline__ TurnScalars turn_prelude(const DevScalars *s, int ring_phase)
{
    static_assert(K == 0 || K == 2, "p in place or two p buffers");
    TurnScalars t;
    t.seq = s->launch_seq;
    t.stopped = s->stop;
    t.rho = s->rho;
    t.norm_factor = s->norm_factor;
    t.init_res = s->init_res;
    t.phase = K > 0 ? ring_phase : 0;
    t.defers = K > 0 && t.phase != 0;
    t.pending = K > 0 ? (unsigned)s->defer_valid : 0u;
    t.t1 = K > 0 ? s->t_ring[1] : 0.0;
    t.iter = s->iter;
    t.n_evals = s->n_evals;
    t.crit = load_criterion(s->crit);
    return t;
}

// the kernel's arguments that the body works on
struct TurnArgs {
    int n;
    double *__restrict__ r;
    const double *__restrict__ inv_diag;
    double *p, *p_out;
    double *__restrict__ x;
    DevScalars *s;
    unsigned long long *tagged;
    double *history;
    LeadBox lead;
    const double *p_pend;  // PRing::b[1]
    int early_slots;  // slots whose x a head that updates x writes before the second wait (HeldZ::early_slots)
};

// the LDS of the turn besides zl
struct TurnLds {
    double sh[3];  // beta | prev_rho | rho
    double slot[2 * N_WAVES];
    double lead_words[LEAD_BOX_WORDS / 2];
    int sh_stop;
    int lead_timed_out;
};

// The R + L slots of a workgroup: what it holds of its chunks (q, then z) -- the first R in registers, the next L in LDS
// (zl: L * CHUNK_ROWS doubles; every thread reads and writes its own two words: no barrier).  `i` must be a constant
// once the caller's loop is unrolled: zr[] indexed at run time would go to scratch.
template <int R, int L>
struct TurnSlots {
    double2 zr[R];
    double *zl;
    __device__ __forceinline__ double2 get(int i) const
    {
        if (i < R) return zr[i < R ? i : 0];
        double2 v;
        v.x = zl[(i - R) * CHUNK_ROWS + ROWS_PER_THREAD * threadIdx.x];
        v.y = zl[(i - R) * CHUNK_ROWS + ROWS_PER_THREAD * threadIdx.x + 1];
        return v;
    }
    __device__ __forceinline__ void put(int i, const double2 &v)
    {
        if (i < R) {
            zr[i < R ? i : 0] = v;
        } else {
            zl[(i - R) * CHUNK_ROWS + ROWS_PER_THREAD * threadIdx.x] = v.x;
            zl[(i - R) * CHUNK_ROWS + ROWS_PER_THREAD * threadIdx.x + 1] = v.y;
        }
    }
};

// chunk_of where the slot is a run-time number (the early-x loop): a Src whose chunk_of is bound to unrolled loops --
// the held-q turn's reads a drawn slot's position through a convergent operation, which a rolled loop with a run-time
// bound cannot be unrolled around -- has chunk_of_rolled beside it
template <class Src>
__device__ __forceinline__ auto turn_chunk_rolled(const Src &src, int i, int) -> decltype(src.chunk_of_rolled(i))
{
    return src.chunk_of_rolled(i);
}
template <class Src>
__device__ __forceinline__ int turn_chunk_rolled(const Src &src, int i, long)
{
    return src.chunk_of(i);
}

// the rows of a slot's chunk (a slot that owns nothing: no rows, no loads)
__device__ __forceinline__ RowPair turn_rows(int chunk, int n)
{
    if (chunk >= 0) return my_rows(chunk, n);
    RowPair none;
    none.row = none.n = 0;
    return none;
}

// the rows phase R has asked for ahead of the slot at work: r, 1 / d (its only use in the turn) and, where q is in
// memory, q.  All three go past the caches: nothing reads r between phase R of one turn and phase R of the next -- z stays
// on chip -- and its 16 N bytes would pass through the Infinity Cache between the two uses of p that can share a line there,
// phase S's gather and phase H's read ("Streams of the resident turn")
template <bool Q_HELD>
struct TurnFront {
    double2 r[TURN_AHEAD], d[TURN_AHEAD], q[TURN_AHEAD];
};
template <>
struct TurnFront<true> {
    double2 r[TURN_AHEAD], d[TURN_AHEAD];
};
template <class Src>
__device__ __forceinline__ void turn_ask(const Src &src, const TurnArgs &a, TurnFront<Src::Q_HELD> &f, int i, int d)
{
    const RowPair rp = turn_rows(src.chunk_of(i), a.n);
    f.r[d] = ld2_stream(a.r, rp);
    if constexpr (!Src::Q_HELD) f.q[d] = ld2_stream(src.q, rp);
    f.d[d].x = f.d[d].y = 1.0;
    if (a.inv_diag) f.d[d] = ld2_stream(a.inv_diag, rp);
}
template <class Src>
__device__ __forceinline__ void turn_ask_first(const Src &src, const TurnArgs &a, TurnFront<Src::Q_HELD> &f)
{
#pragma unroll
    for (int d = 0; d < TURN_AHEAD; ++d) turn_ask(src, a, f, d, d);
}

// the first wait: beta = the 16 sums in the mailbox's array 0, left to right (FIN_BETA).  false: a leader never published
// -- comm_error is raised, the kernel leaves
__device__ __forceinline__ bool turn_await_beta(const TurnArgs &a, const TurnScalars &ts, TurnLds &lds, double &beta)
{
    if (!lead_wait(a.lead, 2 * FIN_WAVES, ts.seq, lds.lead_words, &lds.lead_timed_out)) {
        if (threadIdx.x == 0) a.s->comm_error = a.s->stop = 1;
        return false;
    }
    if (threadIdx.x == 0) lds.sh[0] = lead_total(lds.lead_words, 0);
    __syncthreads();
    beta = lds.sh[0];
    return true;
}

// phase R and the sums of its partials
template <int R, int L, class Src>
__device__ __forceinline__ void turn_phase_r(const Src &src, const TurnArgs &a, const TurnScalars &ts, TurnLds &lds,
                                             TurnSlots<R, L> &z, TurnFront<Src::Q_HELD> &f, double beta)
{
    constexpr int D = TURN_AHEAD;
    const int w = blockIdx.x;
    const uint32_t tag = ts.seq + 1;
#pragma unroll
    for (int i = 0; i < R + L; ++i) {
        const int chunk = src.chunk_of(i);
        if (chunk < 0) {  // (workgroup-uniform; no break: the loop must unroll, the slots are indexed at compile time)
            if (i + D < R + L) turn_ask(src, a, f, i + D, i % D);
            continue;
        }
        const RowPair rp = my_rows(chunk, a.n);
        double2 vr = f.r[i % D];
        const double2 vi = f.d[i % D];
        double2 vq;
        if constexpr (!Src::Q_HELD) vq = f.q[i % D];
        if (i + D < R + L) turn_ask(src, a, f, i + D, i % D);
        if constexpr (Src::Q_HELD) vq = z.get(i);
        if (beta != 0.0) {
            const double t = ts.rho / beta;
            vr.x -= t * vq.x;
            vr.y -= t * vq.y;
            st2_stream(a.r, rp, vr);
        }
        double2 vz = vr;
        if (a.inv_diag) {
            vz.x = vr.x * vi.x;
            vz.y = vr.y * vi.y;
        }
        z.put(i, vz);
        double d = 0.0, s = 0.0;
        if (rp.n > 0) {
            d += vr.x * vz.x;
            s += fabs(vr.x);
        }
        if (rp.n > 1) {
            d += vr.y * vz.y;
            s += fabs(vr.y);
        }
        block_sum2(d, s, lds.slot);
        if (threadIdx.x == 0) {
            put_tagged(a.tagged + Src::STRIDE * (size_t)chunk + Src::WORD, tag, d);
            put_tagged(a.tagged + Src::STRIDE * (size_t)chunk + Src::WORD + 2, tag, s);
        }
    }
    // the sums of all partials: workgroup b < 32 is wavefront b % 16 of the finaliser for array b / 16
    // (into arrays 1 and 2 of the mailbox: array 0 keeps beta for a workgroup that still polls for it -- one that owns no
    // chunk holds nobody's sums back)
    if (w < 2 * FIN_WAVES)
        lead_wave_sums_tagged(a.lead, tag, a.tagged + Src::WORD + 2 * (w / FIN_WAVES), Src::STRIDE, src.n_partials,
                              w % FIN_WAVES, 1 + w / FIN_WAVES);
}

// phase H: x, the second wait, the check, the scalars by workgroup 0, p_new
template <int R, int L, int K, class Src>
__device__ __forceinline__ void turn_phase_h(const Src &src, const TurnArgs &a, const TurnScalars &ts, TurnLds &lds,
                                             const TurnSlots<R, L> &z, double beta)
{
    const int w = blockIdx.x;
    const uint32_t tag = ts.seq + 1;
    // this head's term of x and the terms pending before it: ((x + t_1 p_1) + t p), the bits of single updates
    const bool own_term = beta != 0.0;
    const double t_own = own_term ? ts.rho / beta : 0.0;
    auto update_x = [&](const RowPair &rp, const double2 &vp, int upto) {
        const bool pend = K > 1 && 1 < upto && ((ts.pending >> 1) & 1u);
        if (!pend && !own_term) return;
        double2 vx = ld2_stream(a.x, rp);
        if (pend) {
            const double2 v1 = ld2(a.p_pend, rp);
            vx.x += ts.t1 * v1.x;
            vx.y += ts.t1 * v1.y;
        }
        if (own_term) {
            vx.x += t_own * vp.x;
            vx.y += t_own * vp.y;
        }
        st2_stream(a.x, rp, vx);
    };
    // x of the first n_early slots goes out while the sums are awaited, at the price of a second read of their p; the
    // others follow in the last loop, from its one read of p.  (A run-time bound: this loop does not touch the slots.)
    const int n_early = ts.defers ? 0 : min(a.early_slots, R + L);
#pragma unroll 2
    for (int i = 0; i < n_early; ++i) {
        const int chunk = turn_chunk_rolled(src, i, 0);
        if (chunk < 0) continue;
        const RowPair rp = my_rows(chunk, a.n);
        update_x(rp, ld2(a.p, rp), K);
    }
    if (!lead_wait(a.lead, 4 * FIN_WAVES, tag, lds.lead_words, &lds.lead_timed_out, 2 * FIN_WAVES)) {
        if (threadIdx.x == 0) a.s->comm_error = a.s->stop = 1;
        return;
    }
    if (threadIdx.x == 0) {
        // FIN_CG_CHECK: swap(prev_rho, rho) of the previous turn, then the criterion
        const double prev_rho = ts.rho, rho = lead_total(lds.lead_words, 0), norm = lead_total(lds.lead_words, 1);
        const Verdict cv = criterion_verdict(ts.crit, ts.iter, ts.n_evals, ts.init_res, ts.norm_factor, norm,
                                             w == 0 ? a.history : nullptr);
        lds.sh[1] = prev_rho;
        lds.sh[2] = rho;
        lds.sh_stop = cv.stop;
        if (w == 0) {
            DevScalars *s = a.s;
            s->beta = beta;
            s->prev_rho = prev_rho;
            s->rho = rho;
            s->x_pending = 0;
            store_verdict(s, cv);
            s->launch_seq = ts.seq + 2;
            // what is pending after this head (nothing when it has updated x itself or stops)
            s->defer_valid = (ts.defers && !cv.stop) ? (int)(ts.pending | (own_term ? 1u << ts.phase : 0u)) : 0;
            if (ts.defers && own_term) s->t_ring[ts.phase] = t_own;
        }
    }
    __syncthreads();
    const double prev = lds.sh[1], rho = lds.sh[2];
    const int stop = lds.sh_stop;
    const double tmp = (prev == 0.0) ? 0.0 : rho / prev;
#pragma unroll
    for (int i = 0; i < R + L; ++i) {
        const int chunk = src.chunk_of(i);
        if (chunk < 0) continue;
        const RowPair rp = my_rows(chunk, a.n);
        // with two p buffers this is the buffer's last read for a long while: past the caches.  A deferring head reads
        // b[1], which is next read as p_pend a whole turn away; a head that updates x reads b[0], which is never read
        // again -- the next launch overwrites it as its p_out.  In place the store below goes to the same line, which the
        // next launch gathers: plain.  (p_pend in update_x is plain for that reason too: it is b[1], read only by the
        // head whose p_out is b[1])
        double2 vp;
        if constexpr (K > 1)
            vp = ld2_stream(a.p, rp);
        else
            vp = ld2(a.p, rp);
        if (!ts.defers && i >= n_early) update_x(rp, vp, K);
        // a deferring head that ends the solve: what is pending goes in now
        if (ts.defers && stop) update_x(rp, vp, ts.phase);
        if (stop) continue;
        const double2 vz = z.get(i);
        vp.x = vz.x + tmp * vp.x;
        vp.y = vz.y + tmp * vp.y;
        st2(a.p_out, rp, vp);
    }
}

template <int R, int L, int K, class Src>
__device__ __forceinline__ void resident_cg_turn(const Src &src, const TurnArgs &a, const TurnScalars &ts, TurnLds &lds,
                                                 TurnSlots<R, L> &z, TurnFront<Src::Q_HELD> &f, double beta)
{
    turn_phase_r<R, L>(src, a, ts, lds, z, f, beta);
    turn_phase_h<R, L, K>(src, a, ts, lds, z, beta);
}

}  // namespace

}  // namespace ogl
