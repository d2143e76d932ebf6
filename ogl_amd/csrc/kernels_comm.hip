// kernels_comm.hip -- peer-mesh all-reduce and halo exchange kernels (mailboxes over hipIpc)
// (geometry, reduction tree and the -ffp-contract=off rule: device_common.hpp)
#include "device_common.hpp"

namespace ogl {

namespace {

__global__ __launch_bounds__(64) void k_peer_allreduce(PeerArgs pa, double *vals, int n, int32_t *error)
{
    double v0 = 0.0, v1 = 0.0;
    if (threadIdx.x == 0) {
        v0 = vals[0];
        if (n > 1) v1 = vals[1];
    }
    const bool ok = peer_allreduce2(pa, v0, v1);
    if (threadIdx.x == 0) {
        vals[0] = v0;
        if (n > 1) vals[1] = v1;
        if (!ok && error) *error = 1;
    }
}

// ---- halo exchange (PeerHalo, kernels.hpp); T: the values' type, Owner: whose exchange (device_common.hpp) ----
// pack + put + signal in one launch: the last workgroup to finish (atomic ticket) stores the flags, after
// every workgroup's puts have been fenced at system scope.
template <class T, class Owner>
__global__ __launch_bounds__(BLOCK) void k_pack_put_signal(int n_send, const int *__restrict__ send_idxs, PeerHalo P,
                                                           const T *__restrict__ x, Owner own, unsigned *ticket)
{
    if (halo_gated(own)) return;
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < n_send) *halo_put_slot<T>(P, j) = x[send_idxs[j]];
    __shared__ int last;
    halo_signal_last(P, ticket, gridDim.x, &last);
}

// wait + "y += A_non_local recv" + the dot partials of the touched chunks in one launch: one
// workgroup per chunk that holds boundary rows.  Same accumulation order as k_spmv_non_local and
// the same per-chunk tree as k_partials (T = float: as the local kernels of the mixed mode, products of the
// float64 casts), so nothing changes in the bits.
// (W and own come first: behind the twelve other arguments the NDOT = 2 instantiations take 10 SGPRs more)
template <int MODE, int NDOT, class T, class Owner>
__global__ __launch_bounds__(BLOCK) void k_halo_finish(HaloWait W, Owner own, int n_rows,
                                                       const int *__restrict__ chunk_list,
                                                       const int *__restrict__ chunk_row_ptr,
                                                       const int *__restrict__ boundary_rows,
                                                       const int *__restrict__ entry_ptrs, const int *__restrict__ cols,
                                                       const T *__restrict__ vals, const T *recv, T *y, const T *w,
                                                       double *part, double *part_yy)
{
    __shared__ double slot[N_WAVES];
    if (halo_gated(own)) return;
    if (!halo_wait(W, own)) return;  // (y stays the local product)
    const int chunk = chunk_list[blockIdx.x];
    for (int i = chunk_row_ptr[blockIdx.x] + threadIdx.x; i < chunk_row_ptr[blockIdx.x + 1]; i += BLOCK) {
        const int row = boundary_rows[i];
        y[row] = halo_row<MODE>(y[row], entry_ptrs[i], entry_ptrs[i + 1], cols, vals, recv);
    }
    if (NDOT >= 1) {
        __threadfence_block();
        __syncthreads();
        const RowPair rp = my_rows(chunk, n_rows);
        const auto vy = ld2(y, rp), vw = ld2(w, rp);
        double d = 0.0, d2 = 0.0;
        if (rp.n > 0) {
            d += (double)vw.x * (double)vy.x;
            d2 += (double)vy.x * (double)vy.x;
        }
        if (rp.n > 1) {
            d += (double)vw.y * (double)vy.y;
            d2 += (double)vy.y * (double)vy.y;
        }
        const double sm = block_sum(d, slot);
        if (threadIdx.x == 0) part[chunk] = sm;
        if (NDOT >= 2) {
            const double s2 = block_sum(d2, slot);
            if (threadIdx.x == 0) part_yy[chunk] = s2;
        }
    }
}

// peerSafeWait: the single waiting workgroup of a rank
template <class Owner>
__global__ __launch_bounds__(64) void k_halo_wait(HaloWait W, Owner own)
{
    if (halo_gated(own)) return;
    (void)halo_wait(W, own);
}

// y[row] (+/-)= A_non_local(row,:) * recv, continuing the accumulator the local kernel stored.
template <int MODE, class T, class R, class Owner>
__global__ __launch_bounds__(BLOCK) void k_spmv_non_local(int n_boundary, const int *__restrict__ boundary_rows,
                                                          const int *__restrict__ entry_ptrs,
                                                          const int *__restrict__ cols, const T *__restrict__ vals,
                                                          const R *__restrict__ recv, T *__restrict__ y, Owner own)
{
    if (halo_gated(own)) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_boundary) return;
    const int row = boundary_rows[i];
    y[row] = halo_row<MODE>(y[row], entry_ptrs[i], entry_ptrs[i + 1], cols, vals, recv);
}

template <class T, class Owner>
__global__ __launch_bounds__(BLOCK) void k_pack(int n_send, const int *__restrict__ send_idxs, const T *__restrict__ x,
                                                double *__restrict__ send, Owner own)
{
    if (halo_gated(own)) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_send) send[i] = (double)x[send_idxs[i]];
}

__global__ void k_peer_post(unsigned long long *dst, unsigned long long w0, unsigned long long w1,
                            unsigned long long w2, unsigned long long w3)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    __hip_atomic_store(dst + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 3, w3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(dst, w0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void launch_peer_allreduce(hipStream_t st, const PeerArgs &pa, double *vals, int n, int32_t *error)
{
    hipLaunchKernelGGL(k_peer_allreduce, dim3(1), dim3(64), 0, st, pa, vals, n, error);
}

template <class T, class Owner>
void launch_pack_put_signal(hipStream_t st, const DevHalo &H, const PeerHalo &P, const T *x, const Owner &own,
                            unsigned *ticket)
{
    if (H.n_send == 0) return;
    hipLaunchKernelGGL((k_pack_put_signal<T, Owner>), dim3(blocks_for(H.n_send)), dim3(BLOCK), 0, st, H.n_send,
                       H.send_idxs, P, x, own, ticket);
}

template <class T, class Owner>
void launch_halo_finish(hipStream_t st, const DevHalo &H, const T *nl_vals, int mode, int32_t n_rows,
                        const int32_t *chunk_list, const int32_t *chunk_row_ptr, int32_t n_chunks_b, const T *recv, T *y,
                        const SpmvDotsOf<T> &dots, const PeerHalo &P, const Owner &own)
{
    if (n_chunks_b == 0) return;
    const dim3 grid(n_chunks_b), block(BLOCK);
#define OGL_HF(MODE, NDOT)                                                                                       \
    hipLaunchKernelGGL((k_halo_finish<MODE, NDOT, T, Owner>), grid, block, 0, st, P.wait, own, n_rows, chunk_list, \
                       chunk_row_ptr, H.boundary_rows, H.entry_ptrs, H.cols, nl_vals, recv, y, dots.with, dots.part,   \
                       dots.part_yy)
    if (mode == SPMV_RESIDUAL) {
        OGL_HF(SPMV_RESIDUAL, 0);
    } else if (dots.part && dots.part_yy) {
        OGL_HF(SPMV_PLAIN, 2);
    } else if (dots.part) {
        OGL_HF(SPMV_PLAIN, 1);
    } else {
        OGL_HF(SPMV_PLAIN, 0);
    }
#undef OGL_HF
}

template <class Owner>
void launch_halo_wait(hipStream_t st, const PeerHalo &P, const Owner &own)
{
    if (P.wait.n_neigh == 0) return;
    hipLaunchKernelGGL(k_halo_wait<Owner>, dim3(1), dim3(64), 0, st, P.wait, own);
}

template <class T, class R, class Owner>
void launch_spmv_non_local(hipStream_t st, const DevHalo &H, const T *nl_vals, int mode, const R *recv, T *y,
                           const Owner &own)
{
    if (H.n_boundary_rows == 0) return;
    const dim3 grid(blocks_for(H.n_boundary_rows)), block(BLOCK);
    if (mode == SPMV_RESIDUAL)
        hipLaunchKernelGGL((k_spmv_non_local<SPMV_RESIDUAL, T, R, Owner>), grid, block, 0, st, H.n_boundary_rows,
                           H.boundary_rows, H.entry_ptrs, H.cols, nl_vals, recv, y, own);
    else
        hipLaunchKernelGGL((k_spmv_non_local<SPMV_PLAIN, T, R, Owner>), grid, block, 0, st, H.n_boundary_rows,
                           H.boundary_rows, H.entry_ptrs, H.cols, nl_vals, recv, y, own);
}

template <class T, class Owner>
void launch_pack(hipStream_t st, const DevHalo &H, const T *x, double *send, const Owner &own)
{
    if (H.n_send == 0) return;
    hipLaunchKernelGGL((k_pack<T, Owner>), dim3(blocks_for(H.n_send)), dim3(BLOCK), 0, st, H.n_send, H.send_idxs, x,
                       send, own);
}

// the two owners of an exchange: the double path, and the inner product of the mixed mode (4-byte values on the peer mesh,
// widened doubles through Comm::exchange).  One dispatcher serves both, so the float set holds three kernels that the
// mixed mode never launches: its product is SPMV_PLAIN with at most one partial array.
#define OGL_HALO_LAUNCHES(T, Owner)                                                                                    \
    template void launch_pack_put_signal(hipStream_t, const DevHalo &, const PeerHalo &, const T *, const Owner &,     \
                                         unsigned *);                                                                  \
    template void launch_halo_finish(hipStream_t, const DevHalo &, const T *, int, int32_t, const int32_t *,           \
                                     const int32_t *, int32_t, const T *, T *, const SpmvDotsOf<T> &, const PeerHalo &, \
                                     const Owner &);                                                                   \
    template void launch_halo_wait(hipStream_t, const PeerHalo &, const Owner &);                                      \
    template void launch_spmv_non_local(hipStream_t, const DevHalo &, const T *, int, const T *, T *, const Owner &);  \
    template void launch_pack(hipStream_t, const DevHalo &, const T *, double *, const Owner &);
OGL_HALO_LAUNCHES(double, HaloOwner)
OGL_HALO_LAUNCHES(float, MixedHaloOwner)
template void launch_spmv_non_local(hipStream_t, const DevHalo &, const float *, int, const double *, float *,
                                    const MixedHaloOwner &);
#undef OGL_HALO_LAUNCHES

void launch_peer_post(hipStream_t st, unsigned long long *dst, unsigned long long w0,
                      unsigned long long w1, unsigned long long w2, unsigned long long w3)
{
    hipLaunchKernelGGL(k_peer_post, dim3(1), dim3(64), 0, st, dst, w0, w1, w2, w3);
}

}  // namespace ogl
