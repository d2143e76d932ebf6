// kernels_factor.hip -- incomplete factorisations IC(0) / ILU(0) on the local matrix in the caller's numbering, their
// exact triangular solves by level schedule, and the Richardson sweeps of IRILU (kernels.hpp: DevFactor, DevTri).
// Operation order is fixed (incomplete factorisations): rows in ascending index, entries in ascending column,
// products and sums rounded separately (-ffp-contract=off), so the result equals a sequential walk bit for bit.
// No kernel waits for another workgroup: a level is one launch, a run of thin levels one single-workgroup launch.
// Keywords factorSweeps (the factor from synchronous fixed-point sweeps, one launch each) and triangularSolves isai (the
// approximate inverses of the two triangles, applied as sparse products): DESIGN.md section 7a.
#include "device_common.hpp"

namespace ogl {

namespace {

__global__ __launch_bounds__(BLOCK) void k_factor_gather(int nf, const int *__restrict__ map_ptr,
                                                         const int *__restrict__ map, const double *__restrict__ src,
                                                         double *__restrict__ f)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= nf) return;
    const int a = map_ptr[e], b = map_ptr[e + 1];
    double s = src[map[a]];
    for (int t = a + 1; t < b; ++t) s += src[map[t]];  // (a column repeated by a cyclic patch)
    f[e] = s;
}

// IC(0) / ILU(0) of row i (the rows it depends on are final)
__device__ __forceinline__ void factor_row(const DevFactor &F, int i)
{
    double *__restrict__ v = F.vals;
    const int r0 = F.row_ptrs[i], d = F.diag[i];
    if (F.ic) {
        for (int e = r0; e < d; ++e) {  // l_ij = (a_ij - sum_k<j l_ik l_jk) / l_jj
            double s = v[e];
            for (int t = F.upd_ptr[e]; t < F.upd_ptr[e + 1]; ++t) s = s - v[F.upd_a[t]] * v[F.upd_b[t]];
            v[e] = s / v[F.diag[F.cols[e]]];
        }
        double s = v[d];
        for (int e = r0; e < d; ++e) s = s - v[e] * v[e];
        if (!(s > 0.0)) atomicMin(F.breakdown, i);
        v[d] = sqrt(s);
    } else {
        for (int e = r0; e < d; ++e) {  // l_ik = a_ik / u_kk, then a_ij -= l_ik u_kj for the j > k row i has
            const double l = v[e] / v[F.diag[F.cols[e]]];
            v[e] = l;
            for (int t = F.upd_ptr[e]; t < F.upd_ptr[e + 1]; ++t) v[F.upd_a[t]] = v[F.upd_a[t]] - l * v[F.upd_b[t]];
        }
        if (!(fabs(v[d]) > 0.0)) atomicMin(F.breakdown, i);
    }
}

__global__ __launch_bounds__(BLOCK) void k_factor_level(DevFactor F, const int *__restrict__ rows, int count)
{
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < count) factor_row(F, rows[t]);
}

__global__ __launch_bounds__(BLOCK) void k_factor_thin(DevFactor F, const int *__restrict__ level_ptr,
                                                       const int *__restrict__ rows, int l0, int l1)
{
    for (int l = l0; l < l1; ++l) {
        for (int t = level_ptr[l] + (int)threadIdx.x; t < level_ptr[l + 1]; t += BLOCK) factor_row(F, rows[t]);
        __syncthreads();  // (one workgroup: its waves share the CU's L1, the barrier's fence orders the stores)
    }
}

// keyword factorSweeps: the start values of the fixed-point sweeps, row i
__global__ __launch_bounds__(BLOCK) void k_factor_sweep_start(DevFactor F, const double *__restrict__ a,
                                                              double *__restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= F.n_rows) return;
    const int r0 = F.row_ptrs[i], d = F.diag[i], r1 = F.row_ptrs[i + 1];
    if (F.ic) {
        for (int e = r0; e < d; ++e) out[e] = a[e] / sqrt(a[F.diag[F.cols[e]]]);
        out[d] = sqrt(a[d]);
    } else {
        for (int e = r0; e < d; ++e) out[e] = a[e] / a[F.diag[F.cols[e]]];
        for (int e = d; e < r1; ++e) out[e] = a[e];
    }
}

// one synchronous sweep of row i: every entry from the values of the sweep before (in), its updates in ascending k
template <bool JUDGE>
__global__ __launch_bounds__(BLOCK) void k_factor_sweep(DevFactor F, const int *__restrict__ gs_ptr,
                                                        const int *__restrict__ gs_a, const int *__restrict__ gs_b,
                                                        const double *__restrict__ a, const double *__restrict__ in,
                                                        double *__restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= F.n_rows) return;
    const int r0 = F.row_ptrs[i], d = F.diag[i], r1 = F.row_ptrs[i + 1];
    if (F.ic) {
        for (int e = r0; e < d; ++e) {  // l_ij = (a_ij - sum_m<j l_im l_jm) / l_jj
            double s = a[e];
            for (int t = F.upd_ptr[e]; t < F.upd_ptr[e + 1]; ++t) s = s - in[F.upd_a[t]] * in[F.upd_b[t]];
            out[e] = s / in[F.diag[F.cols[e]]];
        }
        double s = a[d];
        for (int e = r0; e < d; ++e) s = s - in[e] * in[e];
        const double l = sqrt(s);
        out[d] = l;
        if (JUDGE && !(l > 0.0)) atomicMin(F.breakdown, i);
    } else {
        for (int e = r0; e < r1; ++e) {  // s = a_ij - sum_k<min(i,j) l_ik u_kj; l_ij = s / u_jj, u_ij = s
            double s = a[e];
            for (int t = gs_ptr[e]; t < gs_ptr[e + 1]; ++t) s = s - in[gs_a[t]] * in[gs_b[t]];
            out[e] = e < d ? s / in[F.diag[F.cols[e]]] : s;
            if (JUDGE && e == d && !(fabs(s) > 0.0 && fabs(s) <= 1.7976931348623157e308)) atomicMin(F.breakdown, i);
        }
    }
}

// keyword triangularSolves isai: row i of the approximate inverse of triangle T on the row's pattern J, by substitution
// over T(J, J); w is read back by the lane that wrote it
__global__ __launch_bounds__(BLOCK) void k_factor_isai_generate(int n, DevTri T, const int *__restrict__ w_row_ptrs,
                                                                const int *__restrict__ w_cols, double *w)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int *__restrict__ c = T.cols;
    const double *__restrict__ v = T.vals;
    const int a = w_row_ptrs[i], m = w_row_ptrs[i + 1] - a;
    if (T.upper) {  // J[0] = i, upwards: w_t = (delta_t0 - sum_q<t w_q u(J[q], J[t])) / u(J[t], J[t])
        for (int t = 0; t < m; ++t) {
            const int jt = w_cols[a + t];
            double s = t == 0 ? 1.0 : 0.0;
            for (int q = 0; q < t; ++q) {
                const int jq = w_cols[a + q], e1 = T.end[jq];
                int lo = T.beg[jq] + 1, hi = e1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c[mid] < jt) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < e1 && c[lo] == jt) s = s - w[a + q] * v[lo];
            }
            w[a + t] = s / v[T.beg[jt]];
        }
    } else {  // J[m - 1] = i, downwards: w_t = (delta_t,m-1 - sum_q>t w_q l(J[q], J[t])) / l(J[t], J[t])
        for (int t = m - 1; t >= 0; --t) {
            const int jt = w_cols[a + t];
            double s = t == m - 1 ? 1.0 : 0.0;
            for (int q = t + 1; q < m; ++q) {
                const int jq = w_cols[a + q], e1 = T.end[jq];
                int lo = T.beg[jq], hi = e1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c[mid] < jt) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < e1 && c[lo] == jt) s = s - w[a + q] * v[lo];
            }
            w[a + t] = T.unit ? s : s / v[T.end[jt]];
        }
    }
}

// x_i = (b_i - sum_j t_ij x_j) [/ t_ii], j ascending
__device__ __forceinline__ void tri_row(const DevTri &T, int i, const double *b, const int *b_perm, double *x)
{
    const int *__restrict__ c = T.cols;
    const double *__restrict__ v = T.vals;
    double s = b[b_perm ? b_perm[i] : i];
    if (T.upper) {
        const int d = T.beg[i], e1 = T.end[i];
        for (int e = d + 1; e < e1; ++e) s = s - v[e] * x[c[e]];
        x[i] = s / v[d];
    } else {
        const int e1 = T.end[i];
        for (int e = T.beg[i]; e < e1; ++e) s = s - v[e] * x[c[e]];
        x[i] = T.unit ? s : s / v[e1];
    }
}

__global__ __launch_bounds__(BLOCK) void k_tri_level(DevTri T, const int *__restrict__ rows, int count, const double *b,
                                                     const int *__restrict__ b_perm, double *x, const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < count) tri_row(T, rows[t], b, b_perm, x);
}

__global__ __launch_bounds__(BLOCK) void k_tri_thin(DevTri T, const int *__restrict__ level_ptr,
                                                    const int *__restrict__ rows, int l0, int l1, const double *b,
                                                    const int *__restrict__ b_perm, double *x, const DevScalars *gate)
{
    if (gate && gate->stop) return;  // (the same word for every thread: no barrier is left waiting)
    for (int l = l0; l < l1; ++l) {
        for (int t = level_ptr[l] + (int)threadIdx.x; t < level_ptr[l + 1]; t += BLOCK) tri_row(T, rows[t], b, b_perm, x);
        __syncthreads();
    }
}

// x_out_i = x_i + (b_i - sum_j t_ij x_j) * inv_d_i over the row's entries in ascending column, the diagonal included
__global__ __launch_bounds__(BLOCK) void k_tri_sweep(int n, DevTri T, const double *__restrict__ inv_d,
                                                     const double *__restrict__ b, const double *__restrict__ x,
                                                     double *__restrict__ x_out, const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int *__restrict__ c = T.cols;
    const double *__restrict__ v = T.vals;
    const double xi = x[i];
    double s = b[i];
    if (T.upper) {
        const int d = T.beg[i], e1 = T.end[i];
        s = s - v[d] * xi;
        for (int e = d + 1; e < e1; ++e) s = s - v[e] * x[c[e]];
        x_out[i] = xi + s * inv_d[i];
    } else {  // unit diagonal: D = I
        const int e1 = T.end[i];
        for (int e = T.beg[i]; e < e1; ++e) s = s - v[e] * x[c[e]];
        s = s - xi;
        x_out[i] = xi + s;
    }
}

__global__ __launch_bounds__(BLOCK) void k_factor_inv_diag(int n, const int *__restrict__ diag,
                                                           const double *__restrict__ f, double *__restrict__ inv_d)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) inv_d[i] = 1.0 / f[diag[i]];
}

__global__ __launch_bounds__(BLOCK) void k_perm_gather_gated(int n, const int *__restrict__ new_id,
                                                             const double *__restrict__ in, double *__restrict__ out,
                                                             const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = in[new_id[i]];
}

__global__ __launch_bounds__(BLOCK) void k_perm_scatter_gated(int n, const int *__restrict__ new_id,
                                                              const double *__restrict__ in, double *__restrict__ out,
                                                              const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[new_id[i]] = in[i];
}

}  // namespace

void launch_factor_gather(hipStream_t st, int32_t nf, const int32_t *map_ptr, const int32_t *map, const double *src,
                          double *f)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_factor_gather, dim3(blocks_for(nf)), dim3(BLOCK), 0, st, nf, map_ptr, map, src, f);
}

void launch_factor_levels(hipStream_t st, const DevFactor &F, const int32_t *level_ptr_host, const int32_t *level_ptr,
                          const int32_t *level_rows, int32_t l0, int32_t l1, bool thin)
{
    if (thin) {
        hipLaunchKernelGGL(k_factor_thin, dim3(1), dim3(BLOCK), 0, st, F, level_ptr, level_rows, l0, l1);
        return;
    }
    for (int32_t l = l0; l < l1; ++l) {
        const int32_t b = level_ptr_host[l], count = level_ptr_host[l + 1] - b;
        if (count > 0)
            hipLaunchKernelGGL(k_factor_level, dim3(blocks_for(count)), dim3(BLOCK), 0, st, F, level_rows + b, count);
    }
}

void launch_tri_levels(hipStream_t st, const DevTri &T, const int32_t *level_ptr_host, const int32_t *level_ptr,
                       const int32_t *level_rows, int32_t l0, int32_t l1, bool thin, const double *b,
                       const int32_t *b_perm, double *x, const DevScalars *gate)
{
    if (thin) {
        hipLaunchKernelGGL(k_tri_thin, dim3(1), dim3(BLOCK), 0, st, T, level_ptr, level_rows, l0, l1, b, b_perm, x,
                           gate);
        return;
    }
    for (int32_t l = l0; l < l1; ++l) {
        const int32_t b0 = level_ptr_host[l], count = level_ptr_host[l + 1] - b0;
        if (count > 0)
            hipLaunchKernelGGL(k_tri_level, dim3(blocks_for(count)), dim3(BLOCK), 0, st, T, level_rows + b0, count, b,
                               b_perm, x, gate);
    }
}

void launch_tri_sweep(hipStream_t st, int32_t n, const DevTri &T, const double *inv_d, const double *b,
                      const double *x, double *x_out, const DevScalars *gate)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_tri_sweep, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, T, inv_d, b, x, x_out, gate);
}

void launch_factor_sweep_start(hipStream_t st, const DevFactor &F, const double *a, double *out)
{
    if (F.n_rows == 0) return;
    hipLaunchKernelGGL(k_factor_sweep_start, dim3(blocks_for(F.n_rows)), dim3(BLOCK), 0, st, F, a, out);
}

void launch_factor_sweep(hipStream_t st, const DevFactor &F, const int32_t *gs_ptr, const int32_t *gs_a,
                         const int32_t *gs_b, const double *a, const double *in, double *out, bool judge)
{
    if (F.n_rows == 0) return;
    if (judge)
        hipLaunchKernelGGL(k_factor_sweep<true>, dim3(blocks_for(F.n_rows)), dim3(BLOCK), 0, st, F, gs_ptr, gs_a, gs_b, a, in,
                           out);
    else
        hipLaunchKernelGGL(k_factor_sweep<false>, dim3(blocks_for(F.n_rows)), dim3(BLOCK), 0, st, F, gs_ptr, gs_a, gs_b, a, in,
                           out);
}

void launch_factor_isai_generate(hipStream_t st, int32_t n, const DevTri &T, const int32_t *w_row_ptrs,
                                 const int32_t *w_cols, double *w_vals)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_factor_isai_generate, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, T, w_row_ptrs, w_cols, w_vals);
}

void launch_factor_inv_diag(hipStream_t st, int32_t n, const int32_t *diag, const double *f, double *inv_d)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_factor_inv_diag, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, diag, f, inv_d);
}

void launch_factor_gather_perm(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out,
                               const DevScalars *gate)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_perm_gather_gated, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, new_id, in, out, gate);
}

void launch_factor_scatter_perm(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out,
                                const DevScalars *gate)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_perm_scatter_gated, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, new_id, in, out, gate);
}

}  // namespace ogl
