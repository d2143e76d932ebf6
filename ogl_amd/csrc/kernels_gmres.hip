// kernels_gmres.hip -- classical Gram-Schmidt in block form for GKOGMRES (property orthoMethod cgs | cgs2; the contract:
// DESIGN.md section 7d).  One round is two passes over the basis instead of one link per basis vector:
//   k_gmres_multidot      the partials of w . V_j for every j of the turn, one pass over w and V_0 .. V_it
//   k_gmres_fin_h         one workgroup per j: h_j = the sum of its partials in k_finalize's tree -> H(j, it) and h[]
//   k_gmres_block_update  w -= sum_j h_j V_j (j ascending, one rounded product and one rounded difference per term) and, in
//                         the same pass, the partials of w . w (the column's FIN_GMRES_COL) or of w . V_j (cgs2's second round)
//   k_gmres_block_update_held  the same with the partials of w . V_j for up to 32 basis vectors, their rows held in registers
// One workgroup per 512-row chunk, thread t owns rows 2t and 2t + 1; every per-(j, chunk) partial is block_sum's value, so
// the bits are those of k_gmres_mgs' dot product.  No kernel waits for another workgroup: the launches of a turn are ordered
// by the stream.  Every kernel is gated on DevScalars::stop.
// The basis type B is a template parameter (property basisPrecision: DESIGN.md section 7e): a basis stored as floats is
// loaded 8 bytes per vector and lane and widened exactly; every product, sum and tree is the double one.
#include "device_common.hpp"

namespace ogl {

namespace {

constexpr int GS_BATCH = 8;  // basis vectors in flight per thread: 16 B x 8 loads, 8 accumulators

// The chunk's partials of w . V_j, j = j0 .. j0 + cnt - 1 (cnt <= GS_BATCH), into part[j * n_part + chunk]: every sum runs
// through block_sum's tree (wave_sum, then the four wave sums left to right), one barrier pair for the batch.
// `slot`: GS_BATCH * N_WAVES doubles of LDS.
// In two steps: dot_to_slot for every vector b of the batch (v: this thread's rows of it), then slots_to_part.
__device__ __forceinline__ void dot_to_slot(const double2 &v, int b, const double2 &vw, const RowPair &rp, double *slot)
{
    double d = 0.0;
    if (rp.n > 0) d += vw.x * v.x;
    if (rp.n > 1) d += vw.y * v.y;
    d = wave_sum(d);
    if ((threadIdx.x & (WAVE - 1)) == 0) slot[b * N_WAVES + threadIdx.x / WAVE] = d;
}
__device__ __forceinline__ void slots_to_part(int j0, int cnt, double *slot, double *__restrict__ part, int n_part, int chunk)
{
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const double *sl = slot + threadIdx.x * N_WAVES;
        double s = sl[0];
#pragma unroll
        for (int w = 1; w < N_WAVES; ++w) s += sl[w];
        part[(size_t)(j0 + threadIdx.x) * n_part + chunk] = s;
    }
    __syncthreads();
}
// The held kernel uses a vector's pair twice, in the update and in the dot products.  A pair of floats passes through here
// between the two, so that the second use widens it again: otherwise the compiler keeps the doubles of the first use, 4
// VGPRs per vector as for a double basis, instead of the 2 that the floats take.
__device__ __forceinline__ void keep_stored(double2 &) {}
__device__ __forceinline__ void keep_stored(float2 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); }

template <class B>
__device__ __forceinline__ void chunk_dots(const B *__restrict__ V, long ld, int j0, int cnt, const double2 &vw,
                                           const RowPair &rp, double *slot, double *__restrict__ part, int n_part, int chunk)
{
    typename PairOf<B>::type v[GS_BATCH];
#pragma unroll
    for (int b = 0; b < GS_BATCH; ++b)
        if (b < cnt) v[b] = ld2(V + (size_t)(j0 + b) * ld, rp);
#pragma unroll
    for (int b = 0; b < GS_BATCH; ++b)
        if (b < cnt) dot_to_slot(widen2(v[b]), b, vw, rp, slot);
    slots_to_part(j0, cnt, slot, part, n_part, chunk);
}

template <class B>
__global__ __launch_bounds__(BLOCK) void k_gmres_multidot(int n, const double *__restrict__ w, const B *__restrict__ V,
                                                          long ld, int k, double *__restrict__ part, int n_part,
                                                          const DevScalars *gate)
{
    __shared__ double slot[GS_BATCH * N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    const double2 vw = ld2(w, rp);
    for (int j0 = 0; j0 < k; j0 += GS_BATCH) chunk_dots(V, ld, j0, min(GS_BATCH, k - j0), vw, rp, slot, part, n_part, chunk);
}

// h_j = sum of row j of the partial array, in k_finalize's tree (reduce_partials: the same 1024 threads, the same order).
// ADD (cgs2's second round): H(j, it) = H(j, it) + g_j, one rounded sum; h[] receives g_j, what the update applies.
template <bool ADD>
__global__ __launch_bounds__(FIN_BLOCK) void k_gmres_fin_h(const DevScalars *gate, const double *__restrict__ part, int n_part,
                                                           double *__restrict__ h, double *__restrict__ h_col)
{
    __shared__ double slot[FIN_WAVES];
    if (gate && gate->stop) return;
    const int j = blockIdx.x;
    const double *const parts[2] = {part + (size_t)j * n_part, nullptr};
    double r[2];
    reduce_partials<1>(parts, n_part, slot, r);
    if (threadIdx.x == 0) {
        h[j] = r[0];
        h_col[j] = ADD ? h_col[j] + r[0] : r[0];
    }
}

// NORM: the partials of w . w on the updated w (part_out[chunk]).  DOTS: the partials of w . V_j on the updated w
// (part_out[j * n_part + chunk]) -- a row's new w is complete only after its whole loop over j, so the chunk's rows of V are
// read a second time, last read first.  Measured, that second reading costs as much as the first (the rows are not found
// in the L2 of the XCD: DESIGN.md section 7d), so this instantiation runs only beyond GS_HELD_MAX basis vectors; up to there
// k_gmres_block_update_held keeps the rows in registers.
template <bool NORM, bool DOTS, class B>
__global__ __launch_bounds__(BLOCK) void k_gmres_block_update(int n, double *__restrict__ w, const B *__restrict__ V,
                                                              long ld, int k, const double *__restrict__ h,
                                                              double *__restrict__ part_out, int n_part,
                                                              const DevScalars *gate)
{
    __shared__ double slot[GS_BATCH * N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    double2 t = ld2(w, rp);
    for (int j0 = 0; j0 < k; j0 += GS_BATCH) {
        const int cnt = min(GS_BATCH, k - j0);
        typename PairOf<B>::type v[GS_BATCH];
        double hj[GS_BATCH];
#pragma unroll
        for (int b = 0; b < GS_BATCH; ++b)
            if (b < cnt) {
                v[b] = ld2(V + (size_t)(j0 + b) * ld, rp);
                hj[b] = h[j0 + b];
            }
#pragma unroll
        for (int b = 0; b < GS_BATCH; ++b)
            if (b < cnt) {
                const double2 vb = widen2(v[b]);
                t.x -= hj[b] * vb.x;
                t.y -= hj[b] * vb.y;
            }
    }
    st2(w, rp, t);
    if (NORM) {
        double d = 0.0;
        if (rp.n > 0) d += t.x * t.x;
        if (rp.n > 1) d += t.y * t.y;
        const double s0 = block_sum(d, slot);
        if (threadIdx.x == 0) part_out[chunk] = s0;
    }
    if (DOTS) {
        const int n_batches = (k + GS_BATCH - 1) / GS_BATCH;
        for (int b = n_batches - 1; b >= 0; --b)
            chunk_dots(V, ld, b * GS_BATCH, min(GS_BATCH, k - b * GS_BATCH), t, rp, slot, part_out, n_part, chunk);
    }
}

// The update with cgs2's second-round partials for up to KMAX basis vectors: a thread keeps its two rows of every V_j in
// registers (4 VGPRs per vector; a float basis: the floats, 2 VGPRs per vector, widened at each use) from the update to the
// dot products, so V is read once.  All loads are issued before the first use; the arithmetic and the trees are those of
// k_gmres_block_update<false, true>.
template <int KMAX, class B>
__global__ __launch_bounds__(BLOCK) void k_gmres_block_update_held(int n, double *__restrict__ w, const B *__restrict__ V,
                                                                   long ld, int k, const double *__restrict__ h,
                                                                   double *__restrict__ part_out, int n_part,
                                                                   const DevScalars *gate)
{
    static_assert(KMAX % GS_BATCH == 0, "whole batches");
    __shared__ double slot[GS_BATCH * N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    double2 t = ld2(w, rp);
    typename PairOf<B>::type v[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) v[j] = ld2(V + (size_t)j * ld, rp);
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) {
            const double hj = h[j];
            const double2 vj = widen2(v[j]);
            t.x -= hj * vj.x;
            t.y -= hj * vj.y;
        }
    st2(w, rp, t);
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) keep_stored(v[j]);
#pragma unroll
    for (int j0 = 0; j0 < KMAX; j0 += GS_BATCH)
        if (j0 < k) {
#pragma unroll
            for (int b = 0; b < GS_BATCH; ++b)
                if (j0 + b < k) dot_to_slot(widen2(v[j0 + b]), b, t, rp, slot);
            slots_to_part(j0, min(GS_BATCH, k - j0), slot, part_out, n_part, chunk);
        }
}
constexpr int GS_HELD_MAX = 32;  // basis vectors a thread holds (krylovDim 30 and one more); beyond: the second reading


template <class B>
void multidot(hipStream_t st, int32_t n, const double *w, const B *V, int64_t ld, int32_t k, double *part, const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0 || k <= 0) return;
    hipLaunchKernelGGL(k_gmres_multidot<B>, dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, part, nc, gate);
}

template <class B>
void block_update(hipStream_t st, int32_t n, double *w, const B *V, int64_t ld, int32_t k, const double *h, double *part_norm,
                  double *part_dots, const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0 || k <= 0) return;
    if (part_dots && k <= GS_BATCH)
        hipLaunchKernelGGL((k_gmres_block_update_held<GS_BATCH, B>), dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, h,
                           part_dots, nc, gate);
    else if (part_dots && k <= 2 * GS_BATCH)
        hipLaunchKernelGGL((k_gmres_block_update_held<2 * GS_BATCH, B>), dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, h,
                           part_dots, nc, gate);
    else if (part_dots && k <= GS_HELD_MAX)
        hipLaunchKernelGGL((k_gmres_block_update_held<GS_HELD_MAX, B>), dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, h,
                           part_dots, nc, gate);
    else if (part_dots)
        hipLaunchKernelGGL((k_gmres_block_update<false, true, B>), dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, h,
                           part_dots, nc, gate);
    else
        hipLaunchKernelGGL((k_gmres_block_update<true, false, B>), dim3(nc), dim3(BLOCK), 0, st, n, w, V, (long)ld, k, h,
                           part_norm, nc, gate);
}

}  // namespace

void launch_gmres_multidot(hipStream_t st, int32_t n, const double *w, const double *V, int64_t ld, int32_t k, double *part,
                           const DevScalars *gate)
{
    multidot(st, n, w, V, ld, k, part, gate);
}
void launch_gmres_multidot(hipStream_t st, int32_t n, const double *w, const float *V, int64_t ld, int32_t k, double *part,
                           const DevScalars *gate)
{
    multidot(st, n, w, V, ld, k, part, gate);
}

void launch_gmres_fin_h(hipStream_t st, int32_t n, const DevScalars *gate, const double *part, int32_t k, double *h,
                        double *h_col, bool add)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0 || k <= 0) return;
    if (add)
        hipLaunchKernelGGL(k_gmres_fin_h<true>, dim3(k), dim3(FIN_BLOCK), 0, st, gate, part, nc, h, h_col);
    else
        hipLaunchKernelGGL(k_gmres_fin_h<false>, dim3(k), dim3(FIN_BLOCK), 0, st, gate, part, nc, h, h_col);
}

void launch_gmres_block_update(hipStream_t st, int32_t n, double *w, const double *V, int64_t ld, int32_t k, const double *h,
                               double *part_norm, double *part_dots, const DevScalars *gate)
{
    block_update(st, n, w, V, ld, k, h, part_norm, part_dots, gate);
}
void launch_gmres_block_update(hipStream_t st, int32_t n, double *w, const float *V, int64_t ld, int32_t k, const double *h,
                               double *part_norm, double *part_dots, const DevScalars *gate)
{
    block_update(st, n, w, V, ld, k, h, part_norm, part_dots, gate);
}

}  // namespace ogl
