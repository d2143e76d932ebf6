// kernels_mixed.hip -- mixed precision for GKOCG: the fp32 inner CG of an fp64 iterative
// refinement.  Vectors and matrix values of the inner solve are binary32; every scalar is formed in fp64 from the wide
// sums (products of the float64 casts, summed in the loop's reduction tree: device_common.hpp) and rounded once; there is
// no fp32 division or square root.  Geometry as everywhere: one workgroup = one chunk of CHUNK_ROWS rows, thread t owns
// rows 2t, 2t + 1 (one 8-byte load per vector), one partial per chunk.
// (-ffp-contract=off: every fp32 product and every fp32 sum rounds once)
#include <algorithm>
#include <climits>

#include "device_common.hpp"
#include "sym_walk.hpp"

namespace ogl {

namespace {

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (false for NaN)

// out[i] = fl32(map ? src[map[i]] (0 where map[i] < 0) : src[i]); *bad = the smallest i whose value is finite in fp64
// and not in fp32, counted from `base`
__global__ __launch_bounds__(BLOCK) void k_mx_refresh(long n, const int *__restrict__ map, const double *__restrict__ src,
                                                      float *__restrict__ out, int *bad, long base)
{
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
        double v = 0.0;
        if (map) {
            const int k = map[i];
            if (k >= 0) v = src[k];
        } else {
            v = src[i];
        }
        const float f = (float)v;
        out[i] = f;
        if (finite_d(v) && !(fabsf(f) <= 3.402823466e38f)) atomicMin(bad, (int)min(base + i, (long)(INT_MAX - 1)));
    }
}

// ------------------------------------------------------------------------------------------
// the inner SpMV on the fp32 twin of the half storage: k_spmv_sym's row walk itself, instantiated for float (sym_rows,
// sym_walk.hpp: the same loads without the streaming ones, the sum in ascending columns, every row from 0.0f) with the
// partial of pi = wide(p, q)
// ------------------------------------------------------------------------------------------
// EPI (MxEpilogue): what follows the product.  MX_EPI_PI: the inner solve's y and partial.  The others serve the fine level
// of Multigrid's cycle in single precision: gated by the Krylov loop's stop flag, they write y = A x
// (_PLAIN), the sweep x + omega32 ((b - A x) inv_d) (_SWEEP; _SWEEP64: as doubles) or the residual b - A x (_RESIDUAL) --
// the row's own x is in registers already, so no elementwise pass follows the product.
template <int EPI>
__device__ __forceinline__ void mg_epilogue(const MgEpi &e, const RowPair &rp, const float2 &xd, const float2 &acc)
{
    const float2 bv = ld2(e.b, rp);
    float2 o;
    if (EPI == MX_EPI_RESIDUAL) {
        o.x = bv.x - acc.x;
        o.y = bv.y - acc.y;
    } else {
        const float2 dv = ld2(e.inv_d, rp);
        const float w = (float)MG_OMEGA;
        const float u0 = w * ((bv.x - acc.x) * dv.x), u1 = w * ((bv.y - acc.y) * dv.y);
        o.x = xd.x + u0;
        o.y = xd.y + u1;
    }
    if (EPI == MX_EPI_SWEEP64) {
        double2 z;
        z.x = (double)o.x;
        z.y = (double)o.y;
        st2(e.out64, rp, z);
    } else {
        st2(e.out, rp, o);
    }
}

template <int ND, bool FAST, int EPI>
__global__ __launch_bounds__(BLOCK) void k_mx_spmv_sym(int n_rows, int n_chunks, SymOffsets off,
                                                       const uint8_t *__restrict__ mask, const float *__restrict__ planes,
                                                       const float *__restrict__ x, float *__restrict__ y,
                                                       double *__restrict__ part, const MixedScalars *gate,
                                                       const int *__restrict__ block_order, MgEpi epi)
{
    __shared__ double slot[N_WAVES];
    if (EPI == MX_EPI_PI) {
        if (mx_gated(gate)) return;
    } else if (epi.gate && epi.gate->stop) {
        return;
    }
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x);
    if (chunk < 0 || chunk >= n_chunks) return;
    const RowPair rp = my_rows(chunk, n_rows);
    float2 xd;
    const float2 acc = sym_rows<SPMV_PLAIN, float, ND, FAST, false>(chunk, rp, n_rows, off, mask, planes, x, nullptr, xd);
    if (EPI > MX_EPI_PLAIN) {
        mg_epilogue<EPI>(epi, rp, xd, acc);
        return;
    }
    st2(y, rp, acc);
    if (EPI == MX_EPI_PI && part) {
        double d = 0.0;
        if (rp.n > 0) d += (double)xd.x * (double)acc.x;
        if (rp.n > 1) d += (double)xd.y * (double)acc.y;
        const double s = block_sum(d, slot);
        if (threadIdx.x == 0) part[chunk] = s;
    }
}

// ... and on the fp32 value array beside the device CSR (k_spmv_stream's walk: the chunk's entries as 8-byte value and
// column pairs, the products parked in LDS, every thread adds up its rows left to right)
template <int EPI>
__global__ __launch_bounds__(BLOCK) void k_mx_spmv_csr(int n_rows, int n_chunks, const int *__restrict__ row_ptrs,
                                                       const int *__restrict__ cols, const float *__restrict__ vals,
                                                       const float *__restrict__ x, float *__restrict__ y,
                                                       double *__restrict__ part, const MixedScalars *gate, int xgroup,
                                                       const int *__restrict__ block_order, MgEpi epi)
{
    __shared__ __attribute__((aligned(16))) float prod[SPMV_TILE];
    __shared__ double slot[N_WAVES];
    if (EPI == MX_EPI_PI) {
        if (mx_gated(gate)) return;
    } else if (epi.gate && epi.gate->stop) {
        return;
    }
    const int chunk = block_order ? block_order[blockIdx.x] : xcd_chunk(blockIdx.x, xgroup);
    if (chunk < 0 || chunk >= n_chunks) return;
    const int tid = threadIdx.x;
    const int r0 = chunk * CHUNK_ROWS;
    const int r1 = min(r0 + CHUNK_ROWS, n_rows);
    const int nz0 = row_ptrs[r0];
    const int nz1 = row_ptrs[r1];
    const int row = r0 + tid * ROWS_PER_THREAD;
    int rs[ROWS_PER_THREAD + 1];
#pragma unroll
    for (int j = 0; j <= ROWS_PER_THREAD; ++j) rs[j] = row_ptrs[min(row + j, r1)];
    float acc[ROWS_PER_THREAD] = {0.0f, 0.0f};
    constexpr int GROUPS = SPMV_TILE / (BLOCK * 2);
    for (int t0 = nz0 & ~3; t0 < nz1; t0 += SPMV_TILE) {
        float2 va[GROUPS];
        int2 cc[GROUPS];
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int e = t0 + (g * BLOCK + tid) * 2;
            const int ec = e < nz1 ? e : t0;  // clamp: stay inside the (padded) arrays
            va[g] = *reinterpret_cast<const float2 *>(vals + ec);
            cc[g] = *reinterpret_cast<const int2 *>(cols + ec);
        }
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            float2 pr;
            pr.x = va[g].x * x[cc[g].x];
            pr.y = va[g].y * x[cc[g].y];
            *reinterpret_cast<float2 *>(prod + (g * BLOCK + tid) * 2) = pr;
        }
        __syncthreads();
        const int t1 = t0 + SPMV_TILE;
#pragma unroll
        for (int j = 0; j < ROWS_PER_THREAD; ++j) {
            const int kb = max(rs[j], t0), ke = min(rs[j + 1], t1);
            for (int k = kb; k < ke; ++k) acc[j] = acc[j] + prod[k - t0];
        }
        __syncthreads();
    }
    if (EPI > MX_EPI_PLAIN) {  // (Multigrid's fine level: the epilogue of mg_epilogue, row by row)
#pragma unroll
        for (int j = 0; j < ROWS_PER_THREAD; ++j) {
            const int i = row + j;
            if (i >= r1) continue;
            const float res = epi.b[i] - acc[j];
            if (EPI == MX_EPI_RESIDUAL) {
                epi.out[i] = res;
                continue;
            }
            const float u = (float)MG_OMEGA * (res * epi.inv_d[i]);
            const float o = x[i] + u;
            if (EPI == MX_EPI_SWEEP64)
                epi.out64[i] = (double)o;
            else
                epi.out[i] = o;
        }
        return;
    }
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
        if (row + j < r1) {
            y[row + j] = acc[j];
            if (EPI == MX_EPI_PI && part) d += (double)x[row + j] * (double)acc[j];
        }
    }
    if (EPI == MX_EPI_PI && part) {
        const double s = block_sum(d, slot);
        if (tid == 0) part[chunk] = s;
    }
}

// ------------------------------------------------------------------------------------------
// vector kernels of the inner solve
// ------------------------------------------------------------------------------------------
// O3 + start: r32 = fl32(r / S), z = r32 * inv_d32 (or r32 itself), u = 0; partials of rho = wide(r32, z), tau0 = wide1(r32)
__global__ __launch_bounds__(BLOCK) void k_mx_start(int n, const double *__restrict__ r, const float *__restrict__ inv_d,
                                                    float *__restrict__ r32, float *__restrict__ z, float *__restrict__ u,
                                                    double *__restrict__ part_rho, double *__restrict__ part_tau,
                                                    const MixedScalars *m)
{
    __shared__ double slot[2 * N_WAVES];
    if (m->outer_stop) return;
    const double S = m->S;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    const double2 rd = ld2(r, rp);
    float2 rv, zv, zero;
    rv.x = rp.n > 0 ? (float)(rd.x / S) : 0.0f;
    rv.y = rp.n > 1 ? (float)(rd.y / S) : 0.0f;
    zero.x = zero.y = 0.0f;
    zv = rv;
    if (inv_d) {
        const float2 dv = ld2(inv_d, rp);
        zv.x = rv.x * dv.x;
        zv.y = rv.y * dv.y;
        st2(z, rp, zv);
    }
    st2(r32, rp, rv);
    st2(u, rp, zero);
    double a = 0.0, b = 0.0;
    if (rp.n > 0) {
        a += (double)rv.x * (double)zv.x;
        b += fabs((double)rv.x);
    }
    if (rp.n > 1) {
        a += (double)rv.y * (double)zv.y;
        b += fabs((double)rv.y);
    }
    block_sum2(a, b, slot);
    if (threadIdx.x == 0) {
        part_rho[chunk] = a;
        part_tau[chunk] = b;
    }
}

// step 1: p = z + fl32(rho / rho_prev) p, or p = z (first turn, rho_prev == 0)
__global__ __launch_bounds__(BLOCK) void k_mx_step1(int n, float *__restrict__ p, const float *__restrict__ z,
                                                    const MixedScalars *m)
{
    if (mx_gated(m)) return;
    const int use_beta = m->use_beta;
    const float b32 = m->b32;
    const RowPair rp = my_rows(blockIdx.x, n);
    float2 zv = ld2(z, rp);
    if (use_beta) {
        const float2 pv = ld2(p, rp);
        const float t0 = b32 * pv.x, t1 = b32 * pv.y;
        zv.x = zv.x + t0;
        zv.y = zv.y + t1;
    }
    st2(p, rp, zv);
}

// steps 4 and 5: u += a p, r -= a q, z = r * inv_d32; partials of rho = wide(r, z), tau = wide1(r)
__global__ __launch_bounds__(BLOCK) void k_mx_step2(int n, float *__restrict__ u, float *__restrict__ r,
                                                    const float *__restrict__ p, const float *__restrict__ q,
                                                    const float *__restrict__ inv_d, float *__restrict__ z,
                                                    double *__restrict__ part_rho, double *__restrict__ part_tau,
                                                    const MixedScalars *m)
{
    __shared__ double slot[2 * N_WAVES];
    if (mx_gated(m)) return;
    const float a32 = m->a32;
    const int chunk = blockIdx.x;
    const RowPair rp = my_rows(chunk, n);
    const float2 pv = ld2(p, rp), qv = ld2(q, rp);
    float2 uv = ld2(u, rp), rv = ld2(r, rp);
    const float up0 = a32 * pv.x, up1 = a32 * pv.y, rq0 = a32 * qv.x, rq1 = a32 * qv.y;
    uv.x = uv.x + up0;
    uv.y = uv.y + up1;
    rv.x = rv.x - rq0;
    rv.y = rv.y - rq1;
    st2(u, rp, uv);
    st2(r, rp, rv);
    float2 zv = rv;
    if (inv_d) {
        const float2 dv = ld2(inv_d, rp);
        zv.x = rv.x * dv.x;
        zv.y = rv.y * dv.y;
        st2(z, rp, zv);
    }
    double a = 0.0, b = 0.0;
    if (rp.n > 0) {
        a += (double)rv.x * (double)zv.x;
        b += fabs((double)rv.x);
    }
    if (rp.n > 1) {
        a += (double)rv.y * (double)zv.y;
        b += fabs((double)rv.y);
    }
    block_sum2(a, b, slot);
    if (threadIdx.x == 0) {
        part_rho[chunk] = a;
        part_tau[chunk] = b;
    }
}

// O5: x += S * (double)u, product and sum rounded separately; not after a stop of the outer loop, not when the inner solve
// ended on a non-finite scalar
__global__ __launch_bounds__(BLOCK) void k_mx_add(int n, double *__restrict__ x, const float *__restrict__ u,
                                                  const MixedScalars *m)
{
    if (m->outer_stop || m->inner_nonfinite) return;
    const double S = m->S;
    const RowPair rp = my_rows(blockIdx.x, n);
    const float2 uv = ld2(u, rp);
    double2 xv = ld2(x, rp);
    const double t0 = S * (double)uv.x, t1 = S * (double)uv.y;
    xv.x = xv.x + t0;
    xv.y = xv.y + t1;
    st2(x, rp, xv);
}

// out[new_id[i]] = in[i] (scatter) | out[i] = in[new_id[i]] (gather): ogl_solver_spmv_f32 on a renumbered device copy
__global__ __launch_bounds__(BLOCK) void k_mx_permute(int n, const int *__restrict__ new_id, const float *__restrict__ in,
                                                      float *__restrict__ out, int gather)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (gather)
        out[i] = in[new_id[i]];
    else
        out[new_id[i]] = in[i];
}

// the pi partial of a chunk over the finished q, in the local kernels' tree (several ranks: the boundary chunks again, after
// the halo kernels of kernels_comm.hip have continued q over the non-local entries)
__device__ __forceinline__ void mx_pi_partial(int n_rows, int chunk, const float *x, const float *y, double *part, double *slot)
{
    const RowPair rp = my_rows(chunk, n_rows);
    const float2 xv = ld2(x, rp), yv = ld2(y, rp);
    double d = 0.0;
    if (rp.n > 0) d += (double)xv.x * (double)yv.x;
    if (rp.n > 1) d += (double)xv.y * (double)yv.y;
    const double sum = block_sum(d, slot);
    if (threadIdx.x == 0) part[chunk] = sum;
}

__global__ __launch_bounds__(BLOCK) void k_mx_pi_chunks(int n_rows, const int *__restrict__ chunk_list, const float *x,
                                                        const float *y, double *part, const MixedScalars *gate)
{
    __shared__ double slot[N_WAVES];
    if (mx_gated(gate)) return;
    mx_pi_partial(n_rows, chunk_list[blockIdx.x], x, y, part, slot);
}

// ------------------------------------------------------------------------------------------
// finalisers (one workgroup, the finaliser's tree): scalars in fp64, every quotient rounded once to binary32
// ------------------------------------------------------------------------------------------
// The sums of a finaliser over the ranks, between its reduction and its logic (v: thread 0's).  Peer mesh: inside the
// launch, ((0 + v_0) + v_1) + ... in rank order.  The other rungs: a do_reduce launch leaves the rank's sums in
// MixedScalars::sums, the caller all-reduces them there, a do_logic launch picks them up.  Returns false (to every thread)
// when this launch has no logic to run.
__device__ __forceinline__ bool mx_global_sums(MixedScalars *m, DevScalars *s, const PeerArgs &pa, int do_reduce, int do_logic,
                                               double (&v)[2])
{
    if (do_reduce && !do_logic) {
        if (threadIdx.x == 0) {
            m->sums[0] = v[0];
            m->sums[1] = v[1];
        }
        return false;
    }
    if (!do_reduce) {
        v[0] = m->sums[0];
        v[1] = m->sums[1];
        return true;
    }
    if (pa.world > 1) {
        unsigned waited = 0;
        const bool ok = peer_allreduce2(pa, v[0], v[1], &waited);
        if (threadIdx.x == 0) {
            m->reduce_wait_ticks += waited;
            m->reduce_waits += 1;
            if (!ok) mx_comm_failed(m, s);
        }
        return ok;
    }
    return true;
}

template <int PHASE>
__global__ __launch_bounds__(FIN_BLOCK) void k_mx_fin(MixedScalars *m, DevScalars *s, const double *part0, const double *part1,
                                                      int n_part, PeerArgs pa, int do_reduce, int do_logic)
{
    __shared__ double slot[FIN_WAVES];
    if (m->outer_stop || m->inner_stop) return;
    const double *const parts[2] = {part0, part1};
    double v[2] = {0.0, 0.0};
    if (do_reduce) {
        if (PHASE == MIXED_FIN_PI)
            reduce_partials<1>(parts, n_part, slot, v);
        else
            reduce_partials<2>(parts, n_part, slot, v);
    }
    if (!mx_global_sums(m, s, pa, do_reduce, do_logic, v)) return;
    if (threadIdx.x != 0) return;
    if (PHASE == MIXED_FIN_START) {  // rho = wide(r, z), tau0 = wide1(r); L turns allowed
        m->rho = v[0];
        m->tau0 = v[1];
        m->tau = v[1];
        if (!finite_d(v[0]) || !finite_d(v[1])) {
            m->inner_nonfinite = 1;
            m->inner_stop = 1;
        } else if (m->inner_cap < 1) {
            m->inner_stop = 1;
        }
    } else if (PHASE == MIXED_FIN_PI) {  // pi = wide(p, q); a = fl32(rho / pi)
        const double pi = v[0];
        m->pi = pi;
        if (pi == 0.0) {  // the turn is not counted
            m->inner_stop = 1;
        } else if (!finite_d(pi)) {
            m->inner_turns = m->inner_turns + 1;
            m->inner_nonfinite = 1;
            m->inner_stop = 1;
        } else {
            m->a32 = (float)(m->rho / pi);
        }
    } else {  // rho_prev = rho, rho = wide(r, z), tau = wide1(r); the inner stop gate
        const double rho_prev = m->rho, rho = v[0], tau = v[1];
        const int j = m->inner_turns + 1;
        m->prev_rho = rho_prev;
        m->rho = rho;
        m->tau = tau;
        m->inner_turns = j;
        if (!finite_d(rho) || !finite_d(tau)) {
            m->inner_nonfinite = 1;
            m->inner_stop = 1;
        } else {
            m->use_beta = rho_prev != 0.0 ? 1 : 0;
            if (rho_prev != 0.0) m->b32 = (float)(rho / rho_prev);
            if (tau <= m->theta * m->tau0 || j >= m->inner_cap) m->inner_stop = 1;
        }
    }
}

// O1 + O2: S = sum |r| (the partials of the residual), the check of outer step k, then this step's inner tolerance and
// budget.  `s`: the double path's scalars -- its norm factor is read, its stop flag raised with the outer stop (the outer
// kernels are the double path's own and gate on it).  Next to S the all-reduce carries the number of overflow words set
// (a value not representable in binary32): every rank ends the solve when any rank has one.
__global__ __launch_bounds__(FIN_BLOCK) void k_mx_head(MixedScalars *m, DevScalars *s, const double *part, int n_part,
                                                       double *history, PeerArgs pa, int do_reduce, int do_logic)
{
    __shared__ double slot[FIN_WAVES];
    if (m->outer_stop) return;
    if (s->comm_error) {  // (an exchange or a sum of the double path's kernels between two checks)
        if (threadIdx.x == 0) mx_comm_failed(m, s);
        return;
    }
    const double *const parts[2] = {part, nullptr};
    double v[2] = {0.0, 0.0};
    if (do_reduce) {
        reduce_partials<1>(parts, n_part, slot, v);
        v[1] = (m->bad_coef != INT_MAX ? 1.0 : 0.0) + (m->bad_invd != INT_MAX ? 1.0 : 0.0);
    }
    if (!mx_global_sums(m, s, pa, do_reduce, do_logic, v)) return;
    if (threadIdx.x != 0) return;
    const double S = v[0], S_prev = m->S;
    const int k = m->outer_steps, T = m->total_turns + m->inner_turns;
    const int prev_turns = m->inner_turns;
    const double nf = s->norm_factor;
    m->total_turns = T;
    m->S_prev = S_prev;
    m->S = S;
    m->norm_factor = nf;
    m->bad_global = (int)v[1];
    int stop = 0, reason = 0;
    if (v[1] != 0.0) {  // a value not representable in binary32, here or on another rank: the solve fails
        stop = 1;
        reason = MIXED_STOP_INVALID;
    }
    CritVals c = load_criterion(m->crit);
    c.frequency = 1;
    const int n_evals = m->n_evals;
    const Verdict vd = criterion_verdict(c, T, n_evals, m->init_res, nf, S, nullptr);
    if (vd.evaluated) {
        if (c.export_res && history) history[n_evals] = vd.res;
        m->n_evals = vd.n_evals;
        m->init_res = vd.init_res;
        m->res = vd.res;
    }
    if (!stop && vd.stop) {
        stop = 1;
        const bool met = vd.res < c.tolerance || (c.rel_tol > 0 && vd.res < c.rel_tol * vd.init_res);
        reason = met ? MIXED_STOP_CRITERION : MIXED_STOP_MAX_ITER;
    }
    if (!stop && k >= 1) {
        if (prev_turns == 0) {
            stop = 1;
            reason = MIXED_STOP_BREAKDOWN;
        } else if (S >= S_prev || !finite_d(S)) {
            stop = 1;
            reason = MIXED_STOP_NO_PROGRESS;
        } else if (S == 0.0) {
            stop = 1;
            reason = MIXED_STOP_CRITERION;
        }
    }
    m->inner_turns = 0;
    if (stop) {
        m->outer_stop = 1;
        m->stop_reason = reason;
        s->stop = 1;
        return;
    }
    const double res = S / nf;
    const double want_abs = c.tolerance, want_rel = c.rel_tol * vd.init_res;
    const double nu = (want_abs > want_rel ? want_abs : want_rel) / res;
    const double half_nu = 0.5 * nu, floor_tol = m->inner_rel_tol;
    m->theta = floor_tol > half_nu ? floor_tol : half_nu;
    const int left = c.max_iter - T;
    m->inner_cap = m->inner_max_iter < left ? m->inner_max_iter : left;
    m->outer_steps = k + 1;
    m->inner_stop = 0;
    m->inner_nonfinite = 0;
    m->use_beta = 0;
}

__global__ void k_mx_reset(MixedScalars *m, DevCriterion crit, double inner_rel_tol, int inner_max_iter)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    MixedScalars z{};
    z.crit = crit;
    z.inner_rel_tol = inner_rel_tol;
    z.inner_max_iter = inner_max_iter;
    z.bad_coef = INT_MAX;
    z.bad_invd = INT_MAX;
    *m = z;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void launch_mixed_refresh(hipStream_t st, int64_t n, const int32_t *map, const double *src, float *out, int32_t *bad,
                          int64_t base)
{
    if (n <= 0) return;
    const int64_t blocks = std::min<int64_t>((n + BLOCK - 1) / BLOCK, 8192);
    hipLaunchKernelGGL(k_mx_refresh, dim3((unsigned)blocks), dim3(BLOCK), 0, st, (long)n, map, src, out, bad, (long)base);
}

void launch_mixed_reset(hipStream_t st, MixedScalars *m, const DevCriterion &crit, double inner_rel_tol, int inner_max_iter)
{
    hipLaunchKernelGGL(k_mx_reset, dim3(1), dim3(64), 0, st, m, crit, inner_rel_tol, inner_max_iter);
}

template <int EPI>
static void mx_launch_sym(hipStream_t st, const DevSym &A, const float *planes, const float *x, float *y, double *part,
                          const MixedScalars *gate, const MgEpi &e)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc)), block(BLOCK);
    sym_dispatch(A, [&](const SymOffsets &off, auto nd, auto fast, auto) {
        hipLaunchKernelGGL((k_mx_spmv_sym<decltype(nd)::value, decltype(fast)::value, EPI>), grid, block, 0, st, A.n_rows, nc,
                           off, A.mask, planes, x, y, part, gate, A.block_order, e);
    });
}

template <int EPI>
static void mx_launch_csr(hipStream_t st, const DevCsr &A, const float *vals, const float *x, float *y, double *part,
                          const MixedScalars *gate, const MgEpi &e)
{
    if (A.n_rows == 0) return;
    const int nc = (int)n_chunks(A.n_rows);
    const int xg = A.xcd_group > 0 ? A.xcd_group : XCD_GROUP;
    const dim3 grid(A.block_order ? A.n_blocks : xcd_grid(nc, xg)), block(BLOCK);
    hipLaunchKernelGGL(k_mx_spmv_csr<EPI>, grid, block, 0, st, A.n_rows, nc, A.row_ptrs, A.cols, vals, x, y, part, gate, xg,
                       A.block_order, e);
}

void launch_mixed_spmv_sym(hipStream_t st, const DevSym &A, const float *planes, const float *x, float *y, double *part,
                           const MixedScalars *gate)
{
    mx_launch_sym<MX_EPI_PI>(st, A, planes, x, y, part, gate, MgEpi{});
}

void launch_mixed_spmv_csr(hipStream_t st, const DevCsr &A, const float *vals, const float *x, float *y, double *part,
                           const MixedScalars *gate)
{
    mx_launch_csr<MX_EPI_PI>(st, A, vals, x, y, part, gate, MgEpi{});
}

// (MX_EPI_PLAIN: the product lands in e.out)
void launch_mg_fine_sym(hipStream_t st, const DevSym &A, const float *planes, MxEpilogue epi, const float *x, const MgEpi &e)
{
    switch (epi) {
    case MX_EPI_PLAIN: mx_launch_sym<MX_EPI_PLAIN>(st, A, planes, x, e.out, nullptr, nullptr, e); break;
    case MX_EPI_SWEEP: mx_launch_sym<MX_EPI_SWEEP>(st, A, planes, x, nullptr, nullptr, nullptr, e); break;
    case MX_EPI_RESIDUAL: mx_launch_sym<MX_EPI_RESIDUAL>(st, A, planes, x, nullptr, nullptr, nullptr, e); break;
    case MX_EPI_SWEEP64: mx_launch_sym<MX_EPI_SWEEP64>(st, A, planes, x, nullptr, nullptr, nullptr, e); break;
    default: break;
    }
}

void launch_mg_fine_csr(hipStream_t st, const DevCsr &A, const float *vals, MxEpilogue epi, const float *x, const MgEpi &e)
{
    switch (epi) {
    case MX_EPI_PLAIN: mx_launch_csr<MX_EPI_PLAIN>(st, A, vals, x, e.out, nullptr, nullptr, e); break;
    case MX_EPI_SWEEP: mx_launch_csr<MX_EPI_SWEEP>(st, A, vals, x, nullptr, nullptr, nullptr, e); break;
    case MX_EPI_RESIDUAL: mx_launch_csr<MX_EPI_RESIDUAL>(st, A, vals, x, nullptr, nullptr, nullptr, e); break;
    case MX_EPI_SWEEP64: mx_launch_csr<MX_EPI_SWEEP64>(st, A, vals, x, nullptr, nullptr, nullptr, e); break;
    default: break;
    }
}

void launch_mixed_fin(hipStream_t st, int phase, MixedScalars *m, DevScalars *s, const MixedFinArgs &a)
{
    const dim3 grid(1), block(FIN_BLOCK);
#define OGL_MX_FIN(PHASE)                                                                                              \
    hipLaunchKernelGGL((k_mx_fin<PHASE>), grid, block, 0, st, m, s, a.part[0], a.part[1], a.n_part, a.peer, a.do_reduce, \
                       a.do_logic)
    switch (phase) {
    case MIXED_FIN_HEAD:
        hipLaunchKernelGGL(k_mx_head, grid, block, 0, st, m, s, a.part[0], a.n_part, a.history, a.peer, a.do_reduce, a.do_logic);
        break;
    case MIXED_FIN_START: OGL_MX_FIN(MIXED_FIN_START); break;
    case MIXED_FIN_PI: OGL_MX_FIN(MIXED_FIN_PI); break;
    default: OGL_MX_FIN(MIXED_FIN_RHO); break;
    }
#undef OGL_MX_FIN
}

void launch_mixed_start(hipStream_t st, int32_t n, const double *r, const float *inv_d, float *r32, float *z, float *u,
                        double *part_rho, double *part_tau, MixedScalars *m)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_mx_start, dim3(nc), dim3(BLOCK), 0, st, n, r, inv_d, r32, z, u, part_rho, part_tau, m);
}

void launch_mixed_step1(hipStream_t st, int32_t n, float *p, const float *z, const MixedScalars *m)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_mx_step1, dim3(nc), dim3(BLOCK), 0, st, n, p, z, m);
}

void launch_mixed_step2(hipStream_t st, int32_t n, float *u, float *r, const float *p, const float *q, const float *inv_d,
                        float *z, double *part_rho, double *part_tau, MixedScalars *m)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_mx_step2, dim3(nc), dim3(BLOCK), 0, st, n, u, r, p, q, inv_d, z, part_rho, part_tau, m);
}

void launch_partials_dot_chunks(hipStream_t st, int32_t n, const float *x, const float *y, double *part,
                                const MixedScalars *gate, const int32_t *chunk_list, int32_t n_list)
{
    if (n_list == 0) return;
    hipLaunchKernelGGL(k_mx_pi_chunks, dim3(n_list), dim3(BLOCK), 0, st, n, chunk_list, x, y, part, gate);
}

void launch_mixed_add(hipStream_t st, int32_t n, double *x, const float *u, const MixedScalars *m)
{
    const int nc = (int)n_chunks(n);
    if (nc == 0) return;
    hipLaunchKernelGGL(k_mx_add, dim3(nc), dim3(BLOCK), 0, st, n, x, u, m);
}

void launch_mixed_permute(hipStream_t st, int32_t n, const int32_t *new_id, const float *in, float *out, bool gather)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_mx_permute, dim3(blocks_for(n)), dim3(BLOCK), 0, st, n, new_id, in, out, gather ? 1 : 0);
}

}  // namespace ogl
