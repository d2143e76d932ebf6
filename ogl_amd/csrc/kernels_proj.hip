// kernels_proj.hip -- the initial guess from the last solutions (keyword guessProjection K; the contract: DESIGN.md section
// 7f).  Before a solve, x0 is replaced by x0 + sum_j alpha_j d_j, alpha minimising |r0 - W alpha|_2 over the stored steps
// d_1 .. d_k with W = A D formed anew on the coefficients of this solve:
//   k_proj_gram<KMAX>  one pass over r0 and w_1 .. w_k: the per-chunk partials of S0 = sum |r0|, g_j = w_j . r0 and
//                      G_ij = w_i . w_j (i >= j), a thread's two rows of every w_j held in registers
//   (k_gmres_fin_h)    one workgroup per sum, in k_finalize's tree (launch_gmres_fin_h)
//   k_proj_solve       thread 0: Cholesky with dropping of G, the two triangular solves, h_j = -alpha_j
//   (k_gmres_block_update)  x = x - sum_j h_j d_j, j ascending (launch_gmres_block_update)
//   k_proj_delta       after the solve: the stored step x_final - x0
// One workgroup per 512-row chunk, thread t owns rows 2t and 2t + 1; every per-chunk partial is block_sum's value, so a
// sum has the bits of k_partials' dot product and norm.  No kernel waits for another workgroup: the launches are ordered
// by the stream.  Every kernel is gated on DevScalars::stop like its neighbours (the pre-step runs before the solve resets
// its scalars and passes no gate).
#include "device_common.hpp"

namespace ogl {

namespace {

// The sums of a solve in the order the small solve reads them: S0 | g_0 .. g_(k-1) | G_00 | G_10 G_11 | G_20 ...
__host__ __device__ __forceinline__ int proj_g(int j) { return 1 + j; }
__host__ __device__ __forceinline__ int proj_G(int k, int i, int j) { return 1 + k + i * (i + 1) / 2 + j; }

// The wavefront's sums of CNT values per lane, every one in wave_sum's tree, for a fraction of its shuffles.  At the level
// of distance OFF wave_sum has lane l add its partner's number (lane l ^ OFF) to its own, and the partner add the same two;
// here the pair shares the work: the lane without the bit keeps the first half of the values, its partner the second, and
// each sends the other the half it gives up -- one shuffle for two sums, the same two numbers added (in either order: the
// same bits).  A value's later levels then run among the lanes that kept it, which are partners of each other at every
// smaller distance.  45 values: 23 + 12 + 6 + 3 + 2 + 1 = 47 shuffles instead of 270.  Once one value is left the levels are
// wave_sum's own.  idx: which of the values this lane ends up holding (>= the count: none, a padding zero); plain: the
// distances that were plain levels -- the lanes without any of these bits are one holder per value.
template <int CNT, int OFF>
struct WaveFold {
    template <int M>
    static __device__ __forceinline__ void run(double (&v)[M], int lane, int &idx, int &plain)
    {
        if constexpr (OFF >= 1) {
            if constexpr (CNT > 1) {
                constexpr int HALF = (CNT + 1) / 2;
                const bool upper = (lane & OFF) != 0;
#pragma unroll
                for (int i = 0; i < HALF; ++i) {
                    const double a = v[i];
                    const double b = i + HALF < CNT ? v[i + HALF] : 0.0;
                    const double send = upper ? a : b;
                    const double keep = upper ? b : a;
                    v[i] = keep + __shfl_xor(send, OFF, WAVE);
                }
                if (upper) idx += HALF;
                WaveFold<HALF, OFF / 2>::run(v, lane, idx, plain);
            } else {
                v[0] += __shfl_xor(v[0], OFF, WAVE);
                plain |= OFF;
                WaveFold<1, OFF / 2>::run(v, lane, idx, plain);
            }
        }
    }
};

// All 1 + KMAX + KMAX (KMAX + 1) / 2 sums of the instantiation are formed (a vector beyond k is zero: its loads are not
// issued), so that every index into the registers is a constant; the partials of the sums of the k vectors are written.
template <int KMAX>
__global__ __launch_bounds__(BLOCK) void k_proj_gram(int n, const double *__restrict__ r0, const double *__restrict__ W,
                                                     long ld, int k, double *__restrict__ part, int n_part,
                                                     const DevScalars *gate)
{
    constexpr int M = 1 + KMAX + KMAX * (KMAX + 1) / 2;
    __shared__ double slot[M * N_WAVES];
    if (gate && gate->stop) return;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    const double2 vr = ld2(r0, rp);
    double2 w[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        w[j].x = w[j].y = 0.0;
        if (j < k) w[j] = ld2(W + (size_t)j * ld, rp);
    }
    // a lane's own sum of its rows, as k_partials forms it: from 0, row 2t, then row 2t + 1 (a row that is not there: a zero
    // operand, which adds +0.0 to a sum that is not -0.0 -- the bits of leaving it out)
    double v[M];
    v[0] = (0.0 + fabs(vr.x)) + fabs(vr.y);
#pragma unroll
    for (int i = 0, s = 1; i < KMAX; ++i) {
        v[s++] = (0.0 + w[i].x * vr.x) + w[i].y * vr.y;
#pragma unroll
        for (int j = 0; j <= i; ++j) v[s++] = (0.0 + w[i].x * w[j].x) + w[i].y * w[j].y;
    }
    const int lane = threadIdx.x & (WAVE - 1);
    int idx = 0, plain = 0;
    WaveFold<M, WAVE / 2>::run(v, lane, idx, plain);
    if (idx < M && (lane & plain) == 0) slot[idx * N_WAVES + threadIdx.x / WAVE] = v[0];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < M) {
        const double *sl = slot + t * N_WAVES;
        double s = sl[0];
#pragma unroll
        for (int wv = 1; wv < N_WAVES; ++wv) s += sl[wv];
        int i = 0, base = 1;  // t = 0: S0; else row i of the triangle starts at base: g_i, G_i0 .. G_ii
        while (t >= base + i + 2) base += i++ + 2;
        const int q = t - base;
        if (t == 0 || i < k) part[(size_t)(t == 0 ? 0 : q == 0 ? proj_g(i) : proj_G(k, i, q - 1)) * n_part + chunk] = s;
    }
}

// Cholesky with dropping, tau = 2^-32: every product, difference, quotient and root rounded once.
// sums: S0 | g | G as k_proj_gram orders them.  h_j = -alpha_j (what the update applies), rec = {S0, kept, k}.
__global__ __launch_bounds__(WAVE) void k_proj_solve(int k, const double *__restrict__ sums, double *__restrict__ h,
                                                     double *__restrict__ rec, const DevScalars *gate)
{
    // (in LDS: indexed at run time, which in registers would mean scratch)
    __shared__ double L[PROJ_MAX][PROJ_MAX], y[PROJ_MAX], alpha[PROJ_MAX];
    __shared__ bool kept[PROJ_MAX];
    if (gate && gate->stop) return;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double tau = 1.0 / 4294967296.0;
    for (int j = 0; j < k; ++j) {
        const double gjj = sums[proj_G(k, j, j)];
        double s = gjj;
        for (int m = 0; m < j; ++m)
            if (kept[m]) s = s - L[j][m] * L[j][m];
        kept[j] = s > tau * gjj;
        if (!kept[j]) continue;
        const double ljj = sqrt(s);
        L[j][j] = ljj;
        for (int i = j + 1; i < k; ++i) {
            double t = sums[proj_G(k, i, j)];
            for (int m = 0; m < j; ++m)
                if (kept[m]) t = t - L[i][m] * L[j][m];
            L[i][j] = t / ljj;
        }
    }
    for (int j = 0; j < k; ++j) {
        if (!kept[j]) continue;
        double t = sums[proj_g(j)];
        for (int m = 0; m < j; ++m)
            if (kept[m]) t = t - L[j][m] * y[m];
        y[j] = t / L[j][j];
    }
    int n_kept = 0;
    bool finite = true;
    for (int j = k - 1; j >= 0; --j) {
        alpha[j] = 0.0;
        if (!kept[j]) continue;
        double t = y[j];
        for (int m = j + 1; m < k; ++m)
            if (kept[m]) t = t - L[m][j] * alpha[m];
        alpha[j] = t / L[j][j];
        finite = finite && isfinite(alpha[j]);
        ++n_kept;
    }
    if (!finite) n_kept = 0;
    for (int j = 0; j < k; ++j) h[j] = -(finite ? alpha[j] : 0.0);
    rec[0] = sums[0];
    rec[1] = (double)n_kept;
    rec[2] = (double)k;
}

__global__ __launch_bounds__(BLOCK) void k_proj_delta(int n, const double *__restrict__ x, const double *__restrict__ x0,
                                                      double *__restrict__ d, const DevScalars *gate)
{
    if (gate && gate->stop) return;
    const RowPair rp = my_rows(blockIdx.x, n);
    const double2 a = ld2(x, rp), b = ld2(x0, rp);
    double2 t;
    t.x = a.x - b.x;
    t.y = a.y - b.y;
    st2(d, rp, t);
}

// Keyword guessProjectionCredit: S0 = sum |b - A x0| of the pre-step (rec[0]) into the criterion's state, between the
// scalars' reset and the solve's first check, where criterion_verdict reads it as the numerator of the initial residual.
// Nothing comes back to the host.  No column kept: x is still the caller's guess and the first norm of the solve is that
// residual's own, so nothing is credited -- the plain solve; the same for an S0 that is not finite or not > 0.
__global__ __launch_bounds__(WAVE) void k_proj_credit(const double *__restrict__ rec, DevScalars *s)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double s0 = rec[0];
    s->init_res = (rec[1] >= 1.0 && s0 > 0.0 && isfinite(s0)) ? s0 : 0.0;
}

}  // namespace

int proj_n_sums(int k) { return 1 + k + k * (k + 1) / 2; }

void launch_proj_credit(hipStream_t st, const double *rec, DevScalars *s)
{
    hipLaunchKernelGGL(k_proj_credit, dim3(1), dim3(WAVE), 0, st, rec, s);
}

void launch_proj_gram(hipStream_t st, int32_t n, const double *r0, const double *W, int64_t ld, int32_t k, double *part,
                      const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0 || k <= 0) return;
    if (k <= 4)
        hipLaunchKernelGGL(k_proj_gram<4>, dim3(nc), dim3(BLOCK), 0, st, n, r0, W, (long)ld, k, part, nc, gate);
    else
        hipLaunchKernelGGL(k_proj_gram<8>, dim3(nc), dim3(BLOCK), 0, st, n, r0, W, (long)ld, k, part, nc, gate);
}

void launch_proj_solve(hipStream_t st, int32_t k, const double *sums, double *h, double *rec, const DevScalars *gate)
{
    hipLaunchKernelGGL(k_proj_solve, dim3(1), dim3(WAVE), 0, st, k, sums, h, rec, gate);
}

void launch_proj_delta(hipStream_t st, int32_t n, const double *x, const double *x0, double *d, const DevScalars *gate)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_proj_delta, dim3(nc), dim3(BLOCK), 0, st, n, x, x0, d, gate);
}

}  // namespace ogl
