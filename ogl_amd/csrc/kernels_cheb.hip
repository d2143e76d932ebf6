// kernels_cheb.hip -- preconditioner Chebyshev: z = p(D^-1 A) D^-1 r, p the Chebyshev polynomial of degree `degree` for
// [lambda_max / ratio, lambda_max] (the table: ChebTable, kernels.hpp).
// (geometry, reduction tree and the -ffp-contract=off rule: device_common.hpp; the half storage's row walk: sym_walk.hpp)
//   generation: k_cheb_bound (Gershgorin bound of D^-1 A, a maximum: order-free, hence reproducible), k_cheb_coeffs
//   apply:      k_cheb_first, then `degree` steps -- k_cheb_step_sym on the whole-matrix half storage (product and
//               recurrence in one kernel), or the residual product of the layout in use followed by k_cheb_step
// Every line of the recurrence is one rounded operation, written once (cheb_update) for both step kernels.  No kernel
// waits for another workgroup: a step reads z of other rows from one buffer and writes its own rows of the other.
#include "device_common.hpp"
#include "sym_walk.hpp"

namespace ogl {

namespace {

// One row's quotient (sum_j |a_ij|) / |a_ii|, the sum from 0 in stored order; the maximum of a wavefront goes to the table
// as the bit pattern of a non-negative double (ordered like the numbers).  A quotient that is not finite (a zero diagonal)
// counts as +inf, so that the maximum keeps it whatever the order.
__global__ __launch_bounds__(BLOCK) void k_cheb_bound(int n_rows, const int *__restrict__ row_ptrs,
                                                      const double *__restrict__ vals, const int *__restrict__ diag_pos,
                                                      ChebTable *tab)
{
    const int row = blockIdx.x * BLOCK + threadIdx.x;
    double q = 0.0;
    if (row < n_rows) {
        double s = 0.0;
        for (int k = row_ptrs[row]; k < row_ptrs[row + 1]; ++k) s = s + fabs(vals[k]);
        const int dp = diag_pos[row];
        const double d = dp >= 0 ? vals[dp] : 0.0;
        q = s / fabs(d);
        if (!isfinite(q)) q = __longlong_as_double(0x7ff0000000000000ll);
    }
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) q = fmax(q, __shfl_xor(q, off, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0)
        atomicMax(reinterpret_cast<unsigned long long *>(&tab->lambda_max), (unsigned long long)__double_as_longlong(q));
}

__global__ __launch_bounds__(WAVE) void k_cheb_coeffs(int n_rows, int degree, double ratio, double forced, ChebTable *tab)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double lmax = forced > 0.0 ? forced : tab->lambda_max;
    tab->breakdown = (n_rows > 0 && !(lmax > 0.0 && isfinite(lmax))) ? 1 : 0;
    const double lmin = lmax / ratio;
    const double theta = (lmax + lmin) / 2.0;
    const double delta = (lmax - lmin) / 2.0;
    const double sigma = theta / delta;
    tab->lambda_max = lmax;
    tab->lambda_min = lmin;
    tab->c0 = 1.0 / theta;
    double rho_prev = 1.0 / sigma;
    for (int k = 0; k < degree; ++k) {
        const double rho = 1.0 / (2.0 * sigma - rho_prev);
        tab->a[k] = rho * rho_prev;
        tab->b[k] = (2.0 * rho) / delta;
        rho_prev = rho;
    }
}

__global__ __launch_bounds__(BLOCK) void k_cheb_first(int n, const double *__restrict__ r, const double *__restrict__ w,
                                                      const ChebTable *__restrict__ tab, double *__restrict__ z1,
                                                      const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const RowPair rp = my_rows(blockIdx.x, n);
    const double c0 = tab->c0;
    const double2 vr = ld2(r, rp), vw = ld2(w, rp);
    double2 z;
    z.x = (vr.x * vw.x) * c0;
    z.y = (vr.y * vw.y) * c0;
    st2(z1, rp, z);
}

// z_next = (z + a (z - z_prev)) + b (w t), one rounding per operation
__device__ __forceinline__ double cheb_update(double t, double w, double z, double z_prev, double a, double b)
{
    t = w * t;
    t = b * t;
    double u = z - z_prev;
    u = a * u;
    return (z + u) + t;
}
// the tail both step kernels share: z_prev from z_io (k == 1: zero), the update, the store, the partial of r . z_next
template <bool LAST>
__device__ __forceinline__ void cheb_finish(int chunk, const RowPair &rp, int k, double2 t, double2 z,
                                            const double *__restrict__ w, const ChebTable *__restrict__ tab,
                                            double *__restrict__ z_io, const double *__restrict__ r,
                                            double *__restrict__ dot_part, double *slot)
{
    const double a = tab->a[k - 1], b = tab->b[k - 1];
    const double2 vw = ld2(w, rp);
    double2 zp;
    zp.x = zp.y = 0.0;
    if (k > 1) zp = ld2(z_io, rp);
    double2 out;
    out.x = cheb_update(t.x, vw.x, z.x, zp.x, a, b);
    out.y = cheb_update(t.y, vw.y, z.y, zp.y, a, b);
    st2(z_io, rp, out);
    if (LAST) {
        const double2 vr = ld2(r, rp);
        double d = 0.0;
        if (rp.n > 0) d += vr.x * out.x;
        if (rp.n > 1) d += vr.y * out.y;
        const double s = block_sum(d, slot);
        if (threadIdx.x == 0) dot_part[chunk] = s;
    }
}

// the unfused step: t = r - A z was written by the residual product of the layout in use
template <bool LAST>
__global__ __launch_bounds__(BLOCK) void k_cheb_step(int n, int k, const double *__restrict__ t, const double *__restrict__ w,
                                                     const ChebTable *__restrict__ tab, const double *__restrict__ z,
                                                     double *__restrict__ z_io, const double *__restrict__ r,
                                                     double *__restrict__ dot_part, const DevScalars *gate)
{
    __shared__ double slot[N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    cheb_finish<LAST>(chunk, rp, k, ld2(t, rp), ld2(z, rp), w, tab, z_io, r, dot_part, slot);
}

// the fused step on the whole-matrix half storage, one workgroup per chunk: the row walk of k_spmv_sym<SPMV_RESIDUAL> on
// x = z, b = r leaves t of the lane's two rows and z at the rows themselves in registers; the recurrence and one paired
// store follow.  z_io is only read and written at the lane's own rows, z only read: no workgroup waits for another.
template <int ND, bool FAST, bool STREAM, bool LAST>
__global__ __launch_bounds__(BLOCK) void k_cheb_step_sym(int n_rows, int n_chunks, SymOffsets off,
                                                         const uint8_t *__restrict__ mask,
                                                         const double *__restrict__ planes, int k,
                                                         const double *__restrict__ r, const double *__restrict__ w,
                                                         const ChebTable *__restrict__ tab, const double *__restrict__ z,
                                                         double *__restrict__ z_io, double *__restrict__ dot_part,
                                                         const DevScalars *gate, const int *__restrict__ block_order)
{
    __shared__ double slot[N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const RowPair rp = my_rows(chunk, n_rows);
    double2 zd;
    const double2 t = sym_rows<SPMV_RESIDUAL, double, ND, FAST, STREAM>(chunk, rp, n_rows, off, mask, planes, z, r, zd);
    cheb_finish<LAST>(chunk, rp, k, t, zd, w, tab, z_io, r, dot_part, slot);
}

}  // namespace

void launch_cheb_bound(hipStream_t st, const DevCsr &A, const int32_t *diag_pos, ChebTable *tab)
{
    if (A.n_rows == 0) return;
    hipLaunchKernelGGL(k_cheb_bound, dim3(blocks_for(A.n_rows)), dim3(BLOCK), 0, st, A.n_rows, A.row_ptrs, A.vals, diag_pos,
                       tab);
}

void launch_cheb_coeffs(hipStream_t st, int32_t n_rows, int32_t degree, double ratio, double forced, ChebTable *tab)
{
    hipLaunchKernelGGL(k_cheb_coeffs, dim3(1), dim3(WAVE), 0, st, n_rows, degree, ratio, forced, tab);
}

void launch_cheb_first(hipStream_t st, int32_t n, const double *r, const double *w, const ChebTable *tab, double *z1,
                       const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_cheb_first, dim3(nc), dim3(BLOCK), 0, st, n, r, w, tab, z1, gate);
}

void launch_cheb_step(hipStream_t st, int32_t n, int32_t k, const double *t, const double *w, const ChebTable *tab,
                      const double *z, double *z_io, const double *r, double *dot_part, const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    if (dot_part)
        hipLaunchKernelGGL(k_cheb_step<true>, dim3(nc), dim3(BLOCK), 0, st, n, k, t, w, tab, z, z_io, r, dot_part, gate);
    else
        hipLaunchKernelGGL(k_cheb_step<false>, dim3(nc), dim3(BLOCK), 0, st, n, k, t, w, tab, z, z_io, r, dot_part, gate);
}

void launch_cheb_step_sym(hipStream_t st, const DevSym &A, int32_t k, const double *r, const double *w, const ChebTable *tab,
                          const double *z, double *z_io, double *dot_part, const DevScalars *gate)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto stream) {
        auto go = [&](auto last) {
            hipLaunchKernelGGL((k_cheb_step_sym<decltype(nd)::value, decltype(fast)::value, decltype(stream)::value,
                                                decltype(last)::value>),
                               grid, block, 0, st, A.n_rows, nc, off, A.mask, A.planes, k, r, w, tab, z, z_io, dot_part, gate,
                               A.block_order);
        };
        if (dot_part)
            go(std::true_type{});
        else
            go(std::false_type{});
    });
}

}  // namespace ogl
