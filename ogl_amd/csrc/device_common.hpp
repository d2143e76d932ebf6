// device_common.hpp -- what the gfx950 (CDNA4) kernels of the Krylov inner loop share (kernels_*.hip).
//
// Everything here is HBM-bandwidth bound (SpMV arithmetic intensity 0.134 flop/B), so there is
// no MFMA: the design rules are coalesced 16-byte-per-lane streams, LDS staging of the SpMV
// products, 64-lane shuffle reductions and an XCD-aware block -> row-chunk map.
//
// Geometry (common.hpp): one 256-thread workgroup (4 wavefronts of 64) owns one chunk of
// CHUNK_ROWS = 512 consecutive rows; thread t owns rows chunk*512 + 2t, +1.
//
// Reductions are deterministic (no atomics): a chunk partial is
//     thread sums (rows in order)  ->  64-lane xor tree (32,16,8,4,2,1)  ->  wave0+wave1+wave2+wave3
// and the finaliser (one 1024-thread workgroup) sums the partials: thread t takes partials
// t, t+1024, ... in order, xor tree per wave, then the 16 wave sums left to right.
// oracle/ogl_oracle.c mirrors this tree in its BLOCKED mode so tests can compare bit for bit.
//
// Compiled with -ffp-contract=off: every product and every sum rounds once, like the reference
// executor of Ginkgo on a baseline x86-64 build (no FMA contraction).
#pragma once
#include "kernels.hpp"

namespace ogl {

namespace {

constexpr int N_WAVES = BLOCK / WAVE;

// ------------------------------------------------------------------------------------------
// reduction tree
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// Every thread returns the block total.  `slot` = N_WAVES doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double *slot)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < N_WAVES; ++w) s += slot[w];
    __syncthreads();
    return s;
}

// Two block totals in one pass (same tree for each, one barrier pair instead of two).  `slot` = 2 N_WAVES doubles.
__device__ __forceinline__ void block_sum2(double &a, double &b, double *slot)
{
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) {
        slot[wave] = a;
        slot[N_WAVES + wave] = b;
    }
    __syncthreads();
    double sa = slot[0], sb = slot[N_WAVES];
#pragma unroll
    for (int w = 1; w < N_WAVES; ++w) {
        sa += slot[w];
        sb += slot[N_WAVES + w];
    }
    __syncthreads();
    a = sa;
    b = sb;
}

// Finaliser tree (one workgroup of FIN_BLOCK = 1024 threads = 16 wavefronts): thread t adds
// partials t, t+1024, ... in that order, then the 64-lane xor tree, then the 16 wave sums left to
// right.  The loads of a batch are issued together (they are independent) and only the adds stay
// ordered, so a 10M-row vector (19,683 partials) costs about one memory latency.
constexpr int FIN_BLOCK = 1024;
constexpr int FIN_WAVES = FIN_BLOCK / WAVE;
constexpr int FIN_BATCH = 8;  // (20 = one batch for 10M rows measured no faster)

__device__ __forceinline__ double fin_block_sum(double v, double *slot)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < FIN_WAVES; ++w) s += slot[w];
    __syncthreads();
    return s;
}

// Reduces one or two partial arrays at once (loads of both in flight together).
template <int K>
__device__ __forceinline__ void reduce_partials(const double *const (&part)[2], int m, double *slot,
                                                double (&out)[2])
{
    double s[2] = {0.0, 0.0};
    for (int i0 = threadIdx.x; i0 < m; i0 += FIN_BLOCK * FIN_BATCH) {
        double v[2][FIN_BATCH];
#pragma unroll
        for (int k = 0; k < FIN_BATCH; ++k) {
            const int i = i0 + k * FIN_BLOCK;
#pragma unroll
            for (int a = 0; a < K; ++a) v[a][k] = i < m ? part[a][i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < FIN_BATCH; ++k)
            if (i0 + k * FIN_BLOCK < m) {
#pragma unroll
                for (int a = 0; a < K; ++a) s[a] += v[a][k];
            }
    }
    out[0] = fin_block_sum(s[0], slot);
    out[1] = K > 1 ? fin_block_sum(s[1], slot) : 0.0;
}

// ------------------------------------------------------------------------------------------
// The peer-put halo exchange (PeerHalo, kernels.hpp): every step of the protocol, once
// ------------------------------------------------------------------------------------------
// wait accounting (DevScalars::halo_wait_ticks): the waiting lanes leave their wait in *longest (LDS, zeroed before),
// one thread adds the workgroup's figure to the solve's counters afterwards
__device__ __forceinline__ void note_wait(unsigned *longest, long long t0)
{
    atomicMax(longest, (unsigned)min((long long)0xffffffffll, wall_clock64() - t0));
}

// The poll: lane i < n_neigh waits for neighbour i's flag of exchange W.seq and leaves *timed_out = 1 when it does not
// come.  No barrier in here: the caller has zeroed the two LDS words behind a barrier and reads them behind another.
__device__ __forceinline__ void halo_poll(const HaloWait &W, int *timed_out, unsigned *longest)
{
    if ((int)threadIdx.x < W.n_neigh) {
        const long long t0 = wall_clock64();
        for (;;) {
            const unsigned long long f =
                __hip_atomic_load(W.local_flag + threadIdx.x, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((uint32_t)f == W.seq) break;
            if (wall_clock64() - t0 > W.timeout_ticks) {
                *timed_out = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        note_wait(longest, t0);
    }
}

// Whose exchange (HaloOwner / MixedHaloOwner, kernels.hpp): is the launch gated, and the outcome of a workgroup's wait
// (one thread calls it) -- the wait goes into the solve's counters; a neighbour that did not show up ends the solve on
// every kernel's gate, and the host reports OGL_ERR_COMM.
__device__ __forceinline__ bool mx_gated(const MixedScalars *m) { return m && (m->outer_stop || m->inner_stop); }
// (also a rank's sums that did not arrive: mx_global_sums, kernels_mixed.hip)
__device__ __forceinline__ void mx_comm_failed(MixedScalars *m, DevScalars *s)
{
    m->comm_error = 1;
    m->outer_stop = 1;
    m->inner_stop = 1;
    if (s) s->stop = 1;
}
__device__ __forceinline__ bool halo_gated(const HaloOwner &o) { return o.gate && o.gate->stop; }
__device__ __forceinline__ bool halo_gated(const MixedHaloOwner &o) { return mx_gated(o.gate); }
__device__ __forceinline__ void halo_wait_outcome(const HaloOwner &o, unsigned longest, int timed_out)
{
    atomicAdd(&o.s->halo_wait_ticks, (unsigned long long)longest);
    atomicAdd(&o.s->halo_waits, 1u);
    if (timed_out) {
        o.s->comm_error = 1;
        o.s->stop = 1;
    }
}
__device__ __forceinline__ void halo_wait_outcome(const MixedHaloOwner &o, unsigned longest, int timed_out)
{
    atomicAdd(&o.m->halo_wait_ticks, (unsigned long long)longest);
    atomicAdd(&o.m->halo_waits, 1u);
    if (timed_out) mx_comm_failed(o.m, o.s);
}

// A workgroup's wait for exchange W.seq; true (to every thread) when every neighbour's values have arrived.
template <class Owner>
__device__ __forceinline__ bool halo_wait(const HaloWait &W, const Owner &own)
{
    __shared__ int timed_out;
    __shared__ unsigned waited;
    if (threadIdx.x == 0) {
        timed_out = 0;
        waited = 0;
    }
    __syncthreads();
    halo_poll(W, &timed_out, &waited);
    __syncthreads();
    if (threadIdx.x == 0) halo_wait_outcome(own, waited, timed_out);
    return timed_out == 0;
}

// A boundary row continued over its non-local entries k0 .. k1 - 1 in stored order -- local first, then non-local, as
// distributed::Matrix::apply does; acc: the row's accumulator after the local entries; R: the receive block's type.
// TURN (the merged step_1x + SpMV kernel of a multi-rank GKOCG turn): what the neighbours have put is z, not p -- the
// new p of a halo column is recomputed here from it and the OLD p of that column, which this rank keeps
// (p_new = z + tmp p_old: the expression, scalars and operands of the owner's own update, hence its bits), and left
// behind in the other of two halo-p buffers for the next turn.
template <int MODE, bool TURN = false, class T, class R>
__device__ __forceinline__ T halo_row(T acc, int k0, int k1, const int *cols, const T *vals, const R *recv, T tmp = 0,
                                      const T *ph_in = nullptr, T *ph_out = nullptr)
{
    for (int k = k0; k < k1; ++k) {
        const int c = cols[k];
        T v = (T)recv[c];
        if (TURN) {
            v = v + tmp * ph_in[c];
            ph_out[c] = v;
        }
        const T t = vals[k] * v;
        acc = (MODE == SPMV_RESIDUAL) ? acc - t : acc + t;
    }
    return acc;
}

// Non-local part of a chunk's rows inside the local SpMV kernel (HaloFused, kernels.hpp).  acc0 / acc1: the
// accumulators of this thread's two rows after the local entries; ys: CHUNK_ROWS doubles of LDS that the
// kernel does not need any more.  Workgroup-uniform: chunks without boundary rows return at once.  The accumulators go
// to LDS between the poll and its barrier, while the flags are on their way.
template <int MODE, bool TURN = false>
__device__ __forceinline__ void halo_fused_add(const HaloFused &H, int chunk, double &acc0, double &acc1, double *ys,
                                               double tmp = 0.0, const double *__restrict__ ph_in = nullptr,
                                               double *__restrict__ ph_out = nullptr)
{
    const int b0 = H.chunk_bptr[chunk], b1 = H.chunk_bptr[chunk + 1];
    if (b0 == b1) return;
    __shared__ int halo_timed_out;
    __shared__ unsigned halo_waited;
    if (threadIdx.x == 0) {
        halo_timed_out = 0;
        halo_waited = 0;
    }
    __syncthreads();
    halo_poll(H.wait, &halo_timed_out, &halo_waited);
    ys[ROWS_PER_THREAD * threadIdx.x] = acc0;
    ys[ROWS_PER_THREAD * threadIdx.x + 1] = acc1;
    __syncthreads();
    if (threadIdx.x == 0) halo_wait_outcome(HaloOwner{nullptr, H.s}, halo_waited, halo_timed_out);
    if (halo_timed_out) return;  // a neighbour is gone: the solve ends (y stays the local product)
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        const int li = H.boundary_rows[i] - chunk * CHUNK_ROWS;
        ys[li] = halo_row<MODE, TURN>(ys[li], H.entry_ptrs[i], H.entry_ptrs[i + 1], H.cols, H.vals, H.recv, tmp, ph_in,
                                      ph_out);
    }
    __syncthreads();
    acc0 = ys[ROWS_PER_THREAD * threadIdx.x];
    acc1 = ys[ROWS_PER_THREAD * threadIdx.x + 1];
}

// XCD-aware chunk map.  The dispatcher places block b on XCD b % 8 (MI355X_MICROARCH.md,
// "Workgroup dispatch"); each XCD has a private 4 MiB L2.  Measured on the 216^3 case
// (tools/spmv_tune.hip, profiles/spmv_tune_r01.txt):
//   * one contiguous eighth of the rows per XCD  -> 208 us  (8 separate DRAM fronts)
//   * plain chunk = block                        -> 193 us
//   * groups of 4 consecutive chunks per XCD, all XCDs advancing on ONE front -> 190 us
// so neighbouring rows (the +-1 / +-nx stencil legs) share an L2 while HBM still sees a single
// streaming front.  Purely a speed choice: results do not depend on placement.
// On an irregular pattern (unstructured mesh in RCM order) the group is a launch parameter: with slabs of
// tens of thousands of rows per XCD the window of x a slab gathers from is fetched into ONE L2 instead of
// all eight (DevCsr::xcd_group, profiles/r03_xcd_group.txt).
constexpr int XCD_GROUP = 4;
__device__ __forceinline__ int xcd_chunk(int block, int group = XCD_GROUP)
{
    const int slot = block / N_XCD, xcd = block % N_XCD;
    return (slot / group) * (N_XCD * group) + xcd * group + slot % group;
}
inline int xcd_grid(int n_chunks, int group = XCD_GROUP)
{
    const int q = N_XCD * group;
    return ((n_chunks + q - 1) / q) * q;
}

// ------------------------------------------------------------------------------------------
// chunk-shaped vector kernels: thread t of block `chunk` owns rows chunk*512 + 2t, +1
// ------------------------------------------------------------------------------------------
struct RowPair {
    int row;  // first row
    int n;    // valid rows (0, 1 or 2)
};
__device__ __forceinline__ RowPair my_rows(int chunk, int n_rows)
{
    RowPair r;
    r.row = chunk * CHUNK_ROWS + threadIdx.x * ROWS_PER_THREAD;
    const int left = n_rows - r.row;
    r.n = left >= ROWS_PER_THREAD ? ROWS_PER_THREAD : (left > 0 ? left : 0);
    return r;
}
// the thread's two rows of a vector of doubles (one 16-byte access) or floats (one 8-byte access)
template <class T>
struct PairOf;
template <>
struct PairOf<double> {
    typedef double2 type;
};
template <>
struct PairOf<float> {
    typedef float2 type;
};
template <class T>
__device__ __forceinline__ typename PairOf<T>::type ld2(const T *__restrict__ p, const RowPair &r)
{
    typename PairOf<T>::type v;
    if (r.n == 2) {
        v = *reinterpret_cast<const typename PairOf<T>::type *>(p + r.row);
    } else {
        v.x = r.n == 1 ? p[r.row] : T(0);
        v.y = T(0);
    }
    return v;
}
template <class T>
__device__ __forceinline__ void st2(T *__restrict__ p, const RowPair &r, typename PairOf<T>::type v)
{
    if (r.n == 2)
        *reinterpret_cast<typename PairOf<T>::type *>(p + r.row) = v;
    else if (r.n == 1)
        p[r.row] = v.x;
}
// a pair as doubles: a pair of floats widened exactly (a stored fp32 Krylov basis, property basisPrecision single)
__device__ __forceinline__ double2 widen2(const double2 &v) { return v; }
__device__ __forceinline__ double2 widen2(const float2 &v)
{
    double2 r;
    r.x = (double)v.x;
    r.y = (double)v.y;
    return r;
}
// the same for data that is not touched again this turn (streamed past the caches, so that the vectors the
// next kernel needs stay in the Infinity Cache; +2.5 % turn rate at 216^3 for the x update alone)
__device__ __forceinline__ double2 ld2_stream(const double *__restrict__ p, const RowPair &r)
{
    typedef double d2v __attribute__((ext_vector_type(2)));
    double2 v;
    if (r.n == 2) {
        const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p + r.row));
        v.x = t.x;
        v.y = t.y;
    } else {
        v.x = r.n == 1 ? p[r.row] : 0.0;
        v.y = 0.0;
    }
    return v;
}
// a pair of values of a matrix plane that is read exactly once per launch
__device__ __forceinline__ double2 ld_pair_stream(const double *__restrict__ p)
{
    typedef double d2v __attribute__((ext_vector_type(2)));
    const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p));
    double2 v;
    v.x = t.x;
    v.y = t.y;
    return v;
}
__device__ __forceinline__ void st2_stream(double *__restrict__ p, const RowPair &r, double2 v)
{
    typedef double d2v __attribute__((ext_vector_type(2)));
    if (r.n == 2) {
        d2v t;
        t.x = v.x;
        t.y = v.y;
        __builtin_nontemporal_store(t, reinterpret_cast<d2v *>(p + r.row));
    } else if (r.n == 1) {
        p[r.row] = v.x;
    }
}
static_assert(ROWS_PER_THREAD == 2, "vector kernels are written for two rows per thread");

// Position j of the send list goes to the neighbour whose block of the list holds it: its place in that neighbour's
// receive segment for this rank (values of type T).
template <class T>
__device__ __forceinline__ T *halo_put_slot(const PeerHalo &P, int j)
{
    int i = 0;
    while (i + 1 < P.wait.n_neigh && j >= P.send_off[i + 1]) ++i;
    return P.segment<T>(i) + (j - P.send_off[i]);
}
// The signal behind a workgroup's puts: they are fenced at system scope, the workgroup takes a ticket, and the last of
// the n_groups workgroups that put for this exchange stores the flags (and leaves the ticket at 0 for the next one).
// *last: one LDS word.
__device__ __forceinline__ void halo_signal_last(const PeerHalo &P, unsigned *ticket, unsigned n_groups, int *last)
{
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *last = atomicAdd(ticket, 1u) == n_groups - 1;
        if (*last) *ticket = 0;
    }
    __syncthreads();
    if (*last && (int)threadIdx.x < P.wait.n_neigh) {
        __threadfence_system();
        __hip_atomic_store(P.remote_flag[threadIdx.x], (unsigned long long)P.wait.seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Halo values of the SpMV that follows, put by the kernel that produces them: this chunk's send rows (v0, v1 = the
// two rows of the thread) go straight into the neighbours' receive blocks -- through LDS, the row's owner holds it in
// registers -- and the last such workgroup of the launch raises the flags.  Workgroup-uniform.
__device__ __forceinline__ void halo_put_chunk(const HaloPutFused &put, int chunk, double v0, double v1, double *ps,
                                               int *last)
{
    const int s0 = put.chunk_sptr[chunk], s1 = put.chunk_sptr[chunk + 1];
    if (s0 == s1) return;
    ps[ROWS_PER_THREAD * threadIdx.x] = v0;
    ps[ROWS_PER_THREAD * threadIdx.x + 1] = v1;
    __syncthreads();
    for (int k = s0 + threadIdx.x; k < s1; k += BLOCK) {
        const int j = put.send_pos[k];
        *halo_put_slot<double>(put.P, j) = ps[put.send_idxs[j] - chunk * CHUNK_ROWS];
    }
    halo_signal_last(put.P, put.ticket, (unsigned)put.n_put_chunks, last);
}

constexpr int FIN_VT = FIN_BLOCK / BLOCK;  // virtual finaliser threads per thread
// the partials this thread's virtual threads own (at most one each: n_part <= FIN_BLOCK), asked for early
template <int K>
__device__ __forceinline__ void load_partials_as_finaliser(const double *__restrict__ p0,
                                                           const double *__restrict__ p1, int m,
                                                           double (&pv)[2][FIN_VT])
{
#pragma unroll
    for (int j = 0; j < FIN_VT; ++j) {
        const int i = threadIdx.x + BLOCK * j;
        pv[0][j] = i < m ? p0[i] : 0.0;
        pv[1][j] = (K > 1 && i < m) ? p1[i] : 0.0;
    }
}
template <int K>
__device__ __forceinline__ void reduce_partials_as_finaliser(const double (&pv)[2][FIN_VT], int m, double *lds,
                                                             double (&out)[2])
{
    // virtual thread v = t + 256 j of the finaliser's 1024 sums partials v, v + 1024, ... (here: just v) from 0.0;
    // its wavefront (v / 64 = t / 64 + 4 j) is summed by the xor tree; then the 16 wavefront sums left to right
    const int t = threadIdx.x;
    double s[2][FIN_VT];
#pragma unroll
    for (int j = 0; j < FIN_VT; ++j) {
        const bool has = t + BLOCK * j < m;
        s[0][j] = has ? 0.0 + pv[0][j] : 0.0;
        s[1][j] = (K > 1 && has) ? 0.0 + pv[1][j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < FIN_VT; ++j) {
        if (BLOCK * j >= m) continue;  // (nothing but 0.0 in these virtual wavefronts: their tree gives 0.0)
        s[0][j] = wave_sum(s[0][j]);
        if (K > 1) s[1][j] = wave_sum(s[1][j]);
    }
    if ((t & (WAVE - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < FIN_VT; ++j) {
            lds[t / WAVE + N_WAVES * j] = s[0][j];
            if (K > 1) lds[FIN_WAVES + t / WAVE + N_WAVES * j] = s[1][j];
        }
    }
    __syncthreads();
    double a = lds[0], b = K > 1 ? lds[FIN_WAVES] : 0.0;
#pragma unroll
    for (int w = 1; w < FIN_WAVES; ++w) {
        a += lds[w];
        if (K > 1) b += lds[FIN_WAVES + w];
    }
    out[0] = a;
    out[1] = b;
    __syncthreads();
}
static_assert(FIN_BLOCK % BLOCK == 0 && FIN_WAVES == N_WAVES * (FIN_BLOCK / BLOCK), "virtual finaliser threads");

#ifndef LEAD_SCOPE
#define LEAD_SCOPE __HIP_MEMORY_SCOPE_SYSTEM  // (agent scope on coarse-grained memory measured no faster)
#endif
// ------------------------------------------------------------------------------------------
// Leader finalisation (large single-rank systems; LeadBox, kernels.hpp).  The kernel that CONSUMES a finaliser's scalars
// runs the finaliser itself: its first 16 workgroups -- dispatched first -- are the 16 wavefronts of k_finalize's tree
// (same order of additions, same bits) and publish their sums in an uncached (fine-grained) mailbox; every workgroup
// polls the mailbox, adds the 16 sums and runs the scalar logic on its own copy of the scalars; workgroup 0 stores the
// new scalars for later kernels.  One launch and one dispatch gap fewer per finaliser.  Visibility: the mailbox words
// carry their own tag (the launch sequence number from the INPUT scalar slot, which no workgroup of this launch writes),
// 32 payload bits each, so no fence and no ordering between the words is needed; the partials and the input scalars
// were written by earlier kernels.  (A finaliser folded into the PRODUCER needs a release per workgroup: measured 4 x
// slower, HISTORY r5 item 14; ONE leader workgroup walking all partials in four batches behind the chip's row loads:
// 13 us against the 10 of the launch it replaces, round 6.)
// ------------------------------------------------------------------------------------------
// The finaliser's 16 wavefronts become the first 16 workgroups of the launch ("leaders"; 32 for two arrays: workgroup b is
// wavefront b % 16 of array b / 16): a leader stages the partials of virtual threads 64 w .. 64 w + 63 (partials v,
// v + 1024, ... each) through LDS with all of its 256 threads -- up to 8 loads per thread in ONE memory round trip for
// systems of up to 16.7 M rows, a tile more beyond -- adds them in the finaliser's order (one wavefront), runs the xor
// tree and publishes the sum.  EVERY workgroup then fetches the 16 (x K) sums and adds them left to right itself, as
// the folded kernels of small systems do with their own copies.
constexpr int LEAD_TILE = 32;                  // partials per virtual thread staged at once
constexpr int LEAD_STAGE = LEAD_TILE * WAVE;   // doubles of LDS (16 KB: eight workgroups per CU keep their place)
__device__ __forceinline__ void lead_wave_sums(const LeadBox &L, uint32_t tag, const double *__restrict__ part, int m, int w,
                                               int array, double *stage /* LEAD_STAGE */)
{
    constexpr int LOADS = LEAD_TILE * WAVE / BLOCK;  // per thread and tile
    static_assert(LOADS * BLOCK == LEAD_TILE * WAVE, "a tile is whole loads of the workgroup");
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int per_thread = (m + FIN_BLOCK - 1) / FIN_BLOCK;  // partials of a virtual thread (the last ones may be missing)
    double s = 0.0;
    for (int k0 = 0; k0 < per_thread; k0 += LEAD_TILE) {
        double v[LOADS];
#pragma unroll
        for (int e = 0; e < LOADS; ++e) {
            const int idx = e * BLOCK + t, k = idx / WAVE, ln = idx % WAVE;
            const long i = (long)(w * WAVE + ln) + (long)FIN_BLOCK * (k0 + k);
            v[e] = i < m ? part[i] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < LOADS; ++e) stage[e * BLOCK + t] = v[e];
        __syncthreads();
        if (wave == 0) {
            const int k_end = min(LEAD_TILE, per_thread - k0);
            for (int k = 0; k < k_end; ++k)
                if ((long)(w * WAVE + lane) + (long)FIN_BLOCK * (k0 + k) < m) s += stage[k * WAVE + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        s = wave_sum(s);
        // every replica of the mailbox gets the two half-words (lane r -> replica r): the pollers spread over the
        // replicas, so that 19,683 workgroups do not fetch the same cache lines from one memory channel
        if (lane < LEAD_REPLICAS) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
            unsigned long long *box = L.box + (size_t)lane * LEAD_REPLICA_STRIDE + array * 2 * FIN_WAVES + 2 * w;
            __hip_atomic_store(box, ((unsigned long long)tag << 32) | (uint32_t)bits, __ATOMIC_RELAXED, LEAD_SCOPE);
            __hip_atomic_store(box + 1, ((unsigned long long)tag << 32) | (uint32_t)(bits >> 32), __ATOMIC_RELAXED, LEAD_SCOPE);
        }
    }
}

// word i of the mailbox: [tag : 32 | payload : 32], one atomic 8-byte store / load each (payload: half of a double)
// Threads 0 .. n_words - 1 of a polling workgroup fetch one word each: half-word i of vals[] (the doubles the leaders
// published, in mailbox order); returns (to every thread) false when a leader never published (time-out: a defect, not
// a state of the solve -- the caller raises comm_error and leaves).  `first`: the mailbox word that half-word 0 of vals[] is
// (a kernel that waits twice keeps its second set of sums in words of their own: a workgroup still polling for the first
// set must never find its words overwritten).
__device__ __forceinline__ bool lead_wait(const LeadBox &L, int n_words, uint32_t tag, double *vals, int *timed_out,
                                          int first = 0)
{
    if (threadIdx.x == 0) *timed_out = 0;
    __syncthreads();
    if ((int)threadIdx.x < n_words) {
        const unsigned long long *src = L.box + (size_t)(blockIdx.x % LEAD_REPLICAS) * LEAD_REPLICA_STRIDE + first + threadIdx.x;
        const long long t0 = wall_clock64();
        for (;;) {
            const unsigned long long w = __hip_atomic_load(src, __ATOMIC_RELAXED, LEAD_SCOPE);
            if ((uint32_t)(w >> 32) == tag) {
                reinterpret_cast<uint32_t *>(vals)[threadIdx.x] = (uint32_t)w;
                break;
            }
            if (wall_clock64() - t0 > L.timeout_ticks) {
                *timed_out = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    __syncthreads();
    return *timed_out == 0;
}
// a double as two tagged half-words [tag : 32 | payload : 32] (the held-z / held-q turns; no fence, no order between them)
__device__ __forceinline__ void put_tagged(unsigned long long *w, uint32_t tag, double v)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    __hip_atomic_store(w, ((unsigned long long)tag << 32) | (uint32_t)bits, __ATOMIC_RELAXED, LEAD_SCOPE);
    __hip_atomic_store(w + 1, ((unsigned long long)tag << 32) | (uint32_t)(bits >> 32), __ATOMIC_RELAXED, LEAD_SCOPE);
}

// lead_wave_sums over partials that arrive while it runs: partial i is words stride i, + 1 of `tagged` (put_tagged; the
// caller points `tagged` at its array's pair of words); a word counts once it carries `tag`.  One wavefront, no staging: lane l is virtual thread 64 w + l and
// adds its partials v, v + 1024, ... in that order -- with a grid of FIN_BLOCK workgroups the order in which workgroup v
// produces them -- four at a time, so that only the last four are awaited after the chip's last chunk.  A partial that
// never arrives: nothing is published, and every workgroup's wait for the box runs into its bound.
__device__ __forceinline__ void lead_wave_sums_tagged(const LeadBox &L, uint32_t tag, const unsigned long long *tagged,
                                                      int stride, int m, int w, int array)
{
    constexpr int Q = 4;
    if (threadIdx.x >= WAVE) return;
    const int lane = threadIdx.x;
    const long long t0 = wall_clock64();
    double s = 0.0;
    bool arrived = true;
    for (long i0 = w * WAVE + lane; arrived && i0 < m; i0 += (long)FIN_BLOCK * Q) {
        unsigned long long lo[Q], hi[Q];
        for (;;) {
            bool all = true;
#pragma unroll
            for (int e = 0; e < Q; ++e) {
                const long i = i0 + (long)FIN_BLOCK * e;
                lo[e] = hi[e] = (unsigned long long)tag << 32;
                if (i < m) {
                    lo[e] = __hip_atomic_load(tagged + (size_t)stride * i, __ATOMIC_RELAXED, LEAD_SCOPE);
                    hi[e] = __hip_atomic_load(tagged + (size_t)stride * i + 1, __ATOMIC_RELAXED, LEAD_SCOPE);
                }
            }
#pragma unroll
            for (int e = 0; e < Q; ++e) all = all && (uint32_t)(lo[e] >> 32) == tag && (uint32_t)(hi[e] >> 32) == tag;
            if (all) break;
            if (wall_clock64() - t0 > L.timeout_ticks) {
                arrived = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int e = 0; e < Q; ++e)
            if (i0 + (long)FIN_BLOCK * e < m) s += __longlong_as_double((long long)((hi[e] << 32) | (uint32_t)lo[e]));
    }
    if (!__all(arrived)) return;  // (the whole wavefront: a sum that lacks one lane's partials must not go out)
    s = wave_sum(s);
    if (lane < LEAD_REPLICAS) put_tagged(L.box + (size_t)lane * LEAD_REPLICA_STRIDE + array * 2 * FIN_WAVES + 2 * w, tag, s);
}

// The leaders of a launch that finalises K partial arrays: workgroup b < 16 K is wavefront b % 16 of array b / 16.
template <int K>
__device__ __forceinline__ void lead_leaders(const LeadBox &L, uint32_t tag, const double *__restrict__ p0,
                                             const double *__restrict__ p1, const double *__restrict__ p2, int m,
                                             double *stage)
{
    if ((int)blockIdx.x < K * FIN_WAVES) {
        const int a = blockIdx.x / FIN_WAVES;
        lead_wave_sums(L, tag, a == 0 ? p0 : (a == 1 ? p1 : p2), m, blockIdx.x % FIN_WAVES, a, stage);
    }
}

// the 16 wavefront sums of array a, left to right (fin_block_sum); a rolled loop: one thread per workgroup runs it, and
// its registers would be every thread's (the step kernels live on 8 wavefronts per SIMD)
__device__ __forceinline__ double lead_total(const double *vals, int a)
{
    double sum = vals[a * FIN_WAVES];
#pragma unroll 1
    for (int w = 1; w < FIN_WAVES; ++w) sum += vals[a * FIN_WAVES + w];
    return sum;
}

// ------------------------------------------------------------------------------------------
// The stopping criterion (StoppingCriterion.C:71-151) on values: the one place where it is written out.  k_finalize reaches
// it through criterion_check below; the folded heads (k_cg_step1x_fin, k_cg_turn_sym, k_bicg_fold1, k_bicg_fold3) and the
// resident turn (resident_cg_turn.hpp) call criterion_verdict from their thread 0.
// What stays with the caller, and has to:
//   * it reads the criterion and the scalars FIELD BY FIELD at its top (load_criterion), before its first barrier or
//     publish.  A by-value copy of DevScalars, or a `const DevScalars &` handed down, lives in scratch memory -- that is
//     where k_finalize's scratch comes from, and a folded kernel with scratch costs more to dispatch than the finaliser
//     launch it saves;
//   * in the resident kernels every workgroup has read every field before it publishes its first partial: workgroup 0
//     overwrites the one scalar slot after the sums;
//   * everything around the verdict: sh[] / sh_stop, which workgroup stores, launch_seq, defer_valid / t_ring, BiCGStab's
//     stop_phase / stop_turn / omega.
// ------------------------------------------------------------------------------------------
struct CritVals {
    double tolerance, rel_tol;
    int min_iter, max_iter, frequency, export_res;
};
__device__ __forceinline__ CritVals load_criterion(const DevCriterion &c)
{
    CritVals v;
    v.tolerance = c.tolerance;
    v.rel_tol = c.rel_tol;
    v.min_iter = c.min_iter;
    v.max_iter = c.max_iter;
    v.frequency = c.frequency;
    v.export_res = c.export_res;
    return v;
}
struct Verdict {
    int iter, n_evals;     // after this check
    double init_res, res;  // res: only when evaluated
    bool evaluated;        // the norm was looked at (n_evals, init_res, res are new)
    int stop;
};
// `norm` is sum|r| over all ranks; `history`: null unless the caller is the workgroup that exports -- the store
// history[iter] = res is the only memory access in here.
// `init_res`: the scalars' init_res as the caller found it.  From the first check on that is the criterion's initial
// normalised residual.  AT the first check (iter == 0) it is the one input the keyword guessProjectionCredit adds: sum|r| at
// the guess the caller handed in, put there by k_proj_credit after the scalars' reset, which takes
// the place of `norm` in the initial residual -- and in nothing else; 0, what the reset leaves, means "as before".  Every
// caller already hands the field in, so the credit costs no kernel a load or a register it did not have.
__device__ __forceinline__ Verdict criterion_verdict(const CritVals &c, int iter, int n_evals, double init_res,
                                                     double norm_factor, double norm, double *history)
{
    Verdict v;
    v.iter = iter + 1;  // :143 (and :80, :86)
    v.n_evals = n_evals;
    v.init_res = init_res;
    v.res = 0.0;
    v.stop = 0;
    v.evaluated = false;
    if (iter > 0 && iter < c.min_iter) return v;  // :77-81
    if (iter % c.frequency != 0) return v;        // :84-87
    v.evaluated = true;
    v.n_evals = n_evals + 1;
    double res = norm;
    if (iter == 0) v.init_res = (init_res != 0.0 ? init_res : res) / norm_factor;  // :102-111 (norm_factor set before)
    res /= norm_factor;                                             // :113
    if (c.export_res && history) history[iter] = res;               // :115-117
    v.res = res;                                                    // :119
    if (iter >= c.max_iter) v.stop = 1;                             // :124
    if (res < c.tolerance) v.stop = 1;                              // :128
    if (c.rel_tol > 0 && res < c.rel_tol * v.init_res) v.stop = 1;  // :132-136
    return v;
}
// the verdict's stores, shared by the folded heads: iter always, the norm's three only when evaluated, stop only when set
__device__ __forceinline__ void store_verdict(DevScalars *s, const Verdict &v)
{
    s->iter = v.iter;
    if (v.evaluated) {
        s->n_evals = v.n_evals;
        s->init_res = v.init_res;
        s->res = v.res;
    }
    if (v.stop) s->stop = 1;
}
// the same on k_finalize's private copy of the scalars: load fields, call, store fields -- with the stores it always had
// (n_evals, init_res at the first check, res only when evaluated; stop only when set)
__device__ inline void criterion_check(DevScalars *s, const DevCriterion &c, double norm, double *history)
{
    const int iter = s->iter;
    const Verdict v = criterion_verdict(load_criterion(c), iter, s->n_evals, s->init_res, s->norm_factor, norm, history);
    if (!v.evaluated) {
        s->iter = v.iter;
        return;
    }
    s->n_evals = v.n_evals;
    if (iter == 0) s->init_res = v.init_res;
    s->res = v.res;
    s->iter = v.iter;
    if (v.stop) s->stop = 1;
}

// Peer-write all-reduce (PeerArgs, kernels.hpp).  Called by every thread of a workgroup of >= 64
// threads; v0, v1 are thread 0's local sums on entry and the rank-ordered global sums on return
// (thread 0 only).  Lane (q, e) sends half-word e to rank q and waits for rank q's half-word e.
__device__ __forceinline__ size_t peer_word(int slot, int src, int e)
{
    return ((size_t)slot * PEER_MAX_RANKS + src) * PEER_ELEMS + e;
}
__device__ inline bool peer_allreduce2(const PeerArgs &pa, double &v0, double &v1, unsigned *waited_out = nullptr)
{
    __shared__ unsigned halves[PEER_MAX_RANKS * PEER_ELEMS];
    __shared__ double mine[2];
    __shared__ int timed_out;
    __shared__ unsigned waited;  // the longest mailbox wait of this all-reduce (DevScalars::reduce_wait_ticks)
    if (threadIdx.x == 0) {
        mine[0] = v0;
        mine[1] = v1;
        timed_out = 0;
        waited = 0;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < pa.world * PEER_ELEMS) {
        const int q = t / PEER_ELEMS, e = t % PEER_ELEMS;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(mine[e >> 1]);
        const unsigned half = (e & 1) ? (unsigned)(bits >> 32) : (unsigned)bits;
        const unsigned long long word = ((unsigned long long)pa.seq << 32) | half;
        const int slot = (int)(pa.seq % PEER_SLOTS);
        __hip_atomic_store(pa.box[q] + peer_word(slot, pa.rank, e), word, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long *src = pa.box[pa.rank] + peer_word(slot, q, e);
        const long long t0 = wall_clock64();
        unsigned long long w;
        for (;;) {
            w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((unsigned)(w >> 32) == pa.seq) break;
            if (wall_clock64() - t0 > pa.timeout_ticks) {
                timed_out = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        note_wait(&waited, t0);
        halves[q * PEER_ELEMS + e] = (unsigned)w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (waited_out) *waited_out = waited;
        double s0 = 0.0, s1 = 0.0;
        for (int q = 0; q < pa.world; ++q) {
            const unsigned *h = halves + q * PEER_ELEMS;
            s0 += __longlong_as_double((long long)(((unsigned long long)h[1] << 32) | h[0]));
            s1 += __longlong_as_double((long long)(((unsigned long long)h[3] << 32) | h[2]));
        }
        v0 = s0;
        v1 = s1;
    }
    return timed_out == 0;
}

inline int blocks_for(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }

}  // namespace

}  // namespace ogl
