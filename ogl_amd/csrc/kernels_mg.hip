// kernels_mg.hip -- the Multigrid preconditioner (Preconditioner.H:259-341): generation of an aggregation hierarchy on
// the device and the kernels of one V-cycle.  The contract is this build's restatement of
// [UPSTREAM] Ginkgo's Pgm(deterministic) + Multigrid; products and sums round separately, and no kernel uses an atomic on a value:
// the result does not depend on scheduling.  Generation is fp64; the apply's kernels take their operand type as a template
// argument (double, or float for keyword cyclePrecision single).
//
// A repeated column of a row (cyclic patches) counts as ONE entry whose value is the sum of the repeats in stored order
// (run_sum); the coarse matrices have one entry per column.
#include <hipcub/hipcub.hpp>

#include <cassert>
#include <type_traits>

#include "device_common.hpp"

namespace ogl {

namespace {

constexpr int MG_BLOCK = 256;
inline int mg_grid(int64_t n) { return (int)((n + MG_BLOCK - 1) / MG_BLOCK); }

// value of the entry that starts at position k of a row ending at `end`, repeats of its column included; next = the
// position behind them
__device__ __forceinline__ double run_sum(const int32_t *__restrict__ cols, const double *__restrict__ vals, int k,
                                          int end, int &next)
{
    const int c = cols[k];
    double v = vals[k];
    int e = k + 1;
    while (e < end && cols[e] == c) {
        v = v + vals[e];
        ++e;
    }
    next = e;
    return v;
}

// A(row, col), 0 when the pattern has no such entry (columns ascending per row)
__device__ __forceinline__ double entry_at(const MgCsr &A, int row, int col)
{
    int lo = A.row_ptrs[row];
    const int end = A.row_ptrs[row + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.cols[mid] < col)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= end || A.cols[lo] != col) return 0.0;
    int next;
    return run_sum(A.cols, A.vals, lo, end, next);
}

// ------------------------------------------------------------------------------------------
// generation
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MG_BLOCK) void k_mg_diag(MgCsr A, double *__restrict__ diag, double *__restrict__ inv_d)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const double d = entry_at(A, i, i);
    diag[i] = d;
    if (inv_d) inv_d[i] = 1.0 / d;  // (nullptr: a pass between two kept levels needs the strengths' diagonal only)
}

// aggregation hashed: the tie-breaker of an edge, symmetric in the pair ("hashed ties")
__device__ __forceinline__ uint32_t mg_edge_hash(int i, int j)
{
    const uint32_t a = (uint32_t)(i < j ? i : j), b = (uint32_t)(i < j ? j : i);
    uint32_t h = (a * 0x9E3779B1u) ^ (b * 0x85EBCA6Bu + 0xC2B2AE35u);
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// s[i] = the neighbour of the unaggregated row i with the largest strength among the unaggregated (want == 0) or the
// aggregated (want == 1) ones, ties to the larger column -- HASHED: to the larger mg_edge_hash(i, j) first; -1: none; -2: row i
// is aggregated already
template <bool HASHED>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_strongest(MgCsr A, const double *__restrict__ diag,
                                                           const int32_t *__restrict__ agg, int want,
                                                           int32_t *__restrict__ s)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    if (agg[i] != -1) {
        s[i] = -2;
        return;
    }
    const double di = fabs(diag[i]);
    double best = -1.0;
    uint32_t bh = 0;
    int bj = -1;
    const int end = A.row_ptrs[i + 1];
    for (int k = A.row_ptrs[i]; k < end;) {
        const int j = A.cols[k];
        int next;
        const double a = run_sum(A.cols, A.vals, k, end, next);
        k = next;
        if (j == i || (int)(agg[j] != -1) != want) continue;
        const double w = 0.5 * (fabs(a) + fabs(entry_at(A, j, i)));
        const double dj = fabs(diag[j]);
        const double st = w / (di > dj ? di : dj);
        if (HASHED) {  // (columns ascend: among equal strengths and hashes the later one is the larger column)
            const uint32_t h = mg_edge_hash(i, j);
            if (st > best || (st == best && h >= bh)) {
                best = st;
                bh = h;
                bj = j;
            }
        } else if (st >= best) {
            best = st;
            bj = j;
        }
    }
    s[i] = bj;
}

// the map of several passes composed: comp (fine row -> row of the pass's matrix) becomes fine row -> the pass's coarse row
__global__ __launch_bounds__(MG_BLOCK) void k_mg_compose(int n, const int32_t *__restrict__ cidx, int32_t *__restrict__ comp)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) comp[i] = cidx[comp[i]];
}

// mutual pairs become aggregates rooted at the smaller row; *left += rows still unaggregated
__global__ __launch_bounds__(MG_BLOCK) void k_mg_match(int n, const int32_t *__restrict__ s, int32_t *__restrict__ agg,
                                                       int32_t *left)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    int un = 0;
    if (i < n) {
        const int j = s[i];
        if (j != -2) {
            if (j >= 0 && s[j] == i)
                agg[i] = i < j ? i : j;
            else
                un = 1;
        }
    }
    const int c = __syncthreads_count(un);
    if (threadIdx.x == 0 && c) atomicAdd(left, c);
}

// leftovers: join the aggregate of s[i] as the rounds left it (those rows are not written here), else a singleton root
__global__ __launch_bounds__(MG_BLOCK) void k_mg_join(int n, const int32_t *__restrict__ s, int32_t *agg)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int j = s[i];
    if (j == -2) return;
    agg[i] = j >= 0 ? agg[j] : i;
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_root_flag(int n, const int32_t *__restrict__ agg, int32_t *__restrict__ flag)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) flag[i] = agg[i] == i ? 1 : 0;
}

// cidx[i] = rank of row i's root among the roots; rows[i] = i
__global__ __launch_bounds__(MG_BLOCK) void k_mg_coarse_index(int n, const int32_t *__restrict__ agg,
                                                              const int32_t *__restrict__ incl, int32_t *__restrict__ cidx,
                                                              int32_t *__restrict__ rows)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    cidx[i] = incl[agg[i]] - 1;
    rows[i] = i;
}

// member lists from the rows sorted (stably) by coarse index
__global__ __launch_bounds__(MG_BLOCK) void k_mg_member_ptr(int n, int nc, const int32_t *__restrict__ sorted,
                                                            int32_t *__restrict__ agg_ptr)
{
    const int p = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (p >= n) return;
    if (p == 0 || sorted[p] != sorted[p - 1]) agg_ptr[sorted[p]] = p;
    if (p == n - 1) agg_ptr[nc] = n;
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_keys(MgCsr A, const int32_t *__restrict__ cidx,
                                                      unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const unsigned long long hi = (unsigned long long)(uint32_t)cidx[i] << 32;
    for (int k = A.row_ptrs[i]; k < A.row_ptrs[i + 1]; ++k) keys[k] = hi | (uint32_t)cidx[A.cols[k]];
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_head_flag(int m, const unsigned long long *__restrict__ keys,
                                                           int32_t *__restrict__ flag)
{
    const int p = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (p < m) flag[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

// one coarse entry per run of equal keys, summed in sorted (= ascending (i, stored position)) order
__global__ __launch_bounds__(MG_BLOCK) void k_mg_compact(int m, int nc, const unsigned long long *__restrict__ keys,
                                                         const double *__restrict__ vals, const int32_t *__restrict__ pos,
                                                         int32_t *__restrict__ row_ptrs, int32_t *__restrict__ cols,
                                                         double *__restrict__ out)
{
    const int p = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (p >= m) return;
    if (p == m - 1) row_ptrs[nc] = pos[p];
    const unsigned long long key = keys[p];
    if (p > 0 && keys[p - 1] == key) return;
    const int o = pos[p] - 1;
    double acc = vals[p];
    for (int q = p + 1; q < m && keys[q] == key; ++q) acc = acc + vals[q];
    cols[o] = (int32_t)(uint32_t)key;
    out[o] = acc;
    const int I = (int)(key >> 32);
    if (p == 0 || (int)(keys[p - 1] >> 32) != I) row_ptrs[I] = o;
}

// ---- keyword aggregateCaching ("kept aggregates"): what a full generation leaves of a pass besides
//      its matrix, and the refresh of the pass's values from it ----
__global__ __launch_bounds__(MG_BLOCK) void k_mg_iota(int m, int32_t *__restrict__ idx)
{
    const int p = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (p < m) idx[p] = p;
}

// ptr[o] = the sorted position at which the run of coarse entry o starts (the inverse of the scan `pos` of the head flags),
// ptr[mc] = m
__global__ __launch_bounds__(MG_BLOCK) void k_mg_run_ptr(int m, const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                         int32_t *__restrict__ ptr)
{
    const int p = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (p >= m) return;
    if (flag[p]) ptr[pos[p] - 1] = p;
    if (p == m - 1) ptr[pos[p]] = m;
}

// One coarse entry per thread: the entries of the pass's source matrix that k_mg_compact summed into it, in that kernel's
// order and with its rule (the sum starts from the first term, every addition rounds once).  src[q]: position in the
// source matrix of the entry sorted to q.  STREAM: src and ptr, read once, go past the caches.
template <bool STREAM>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_regalerkin(int mc, const int32_t *__restrict__ ptr,
                                                            const int32_t *__restrict__ src,
                                                            const double *__restrict__ vals_in, double *__restrict__ vals_out)
{
    const int o = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (o >= mc) return;
    const auto once = [](const int32_t *p) { return STREAM ? __builtin_nontemporal_load(p) : *p; };
    int q = once(ptr + o);
    const int end = once(ptr + o + 1);
    double acc = vals_in[once(src + q)];
    for (++q; q < end; ++q) acc = acc + vals_in[once(src + q)];
    vals_out[o] = acc;
}

// ------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------
#define MG_GATE() \
    if (gate && gate->stop) return

// The apply's kernels take their operand type T from the caller: double (the contract of section 7b as it always was), or
// float for `cyclePrecision single` -- the same operations in the same order on binary32 operands, every product and
// every sum rounded once to T; omega is 0.9 rounded to T.  The coarsest CG's scalars are doubles in either case.

// first pre-sweep, from x = 0
template <class T>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_jacobi0(int n, const T *__restrict__ b, const T *__restrict__ inv_d,
                                                         T *__restrict__ x, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) x[i] = (T)MG_OMEGA * (b[i] * inv_d[i]);
}

// ... of level 0 in single precision: b = fl32(r) is formed (and kept) on the way
__global__ __launch_bounds__(MG_BLOCK) void k_mg_jacobi0_in(int n, const double *__restrict__ r,
                                                            const float *__restrict__ inv_d, float *__restrict__ b,
                                                            float *__restrict__ x, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float bi = (float)r[i];
    b[i] = bi;
    x[i] = (float)MG_OMEGA * (bi * inv_d[i]);
}

// z = (double) x
__global__ __launch_bounds__(MG_BLOCK) void k_mg_widen(int n, const float *__restrict__ x, double *__restrict__ out,
                                                       const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) out[i] = (double)x[i];
}

// the binary32 twin of a level: values and 1 / d rounded from the stored doubles; *bad = the smallest row that holds a
// value finite in fp64 and not in binary32
__global__ __launch_bounds__(MG_BLOCK) void k_mg_twin(MgCsr A, const double *__restrict__ inv_d, float *__restrict__ vals32,
                                                      float *__restrict__ inv_d32, int32_t *bad)
{
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    bool over = false;
    const double d = inv_d[i];
    const float fd = (float)d;
    inv_d32[i] = fd;
    over = fabs(d) <= 1.7976931348623157e308 && !(fabsf(fd) <= 3.402823466e38f);
    if (vals32) {
        for (int k = A.row_ptrs[i]; k < A.row_ptrs[i + 1]; ++k) {
            const double v = A.vals[k];
            const float f = (float)v;
            vals32[k] = f;
            over = over || (fabs(v) <= 1.7976931348623157e308 && !(fabsf(f) <= 3.402823466e38f));
        }
    }
    if (over) atomicMin(bad, i);
}

// the sweep behind a product ax = A x that another kernel has formed
__global__ __launch_bounds__(MG_BLOCK) void k_mg_sweep_epi(int n, const double *__restrict__ b, const double *__restrict__ ax,
                                                           const double *__restrict__ inv_d, const double *__restrict__ x,
                                                           double *__restrict__ x_out, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) x_out[i] = x[i] + MG_OMEGA * ((b[i] - ax[i]) * inv_d[i]);
}

// x_out = x + scale xc[agg] (keyword correctionScale; the product rounded once, then the sum)
template <class T>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_prolong(int n, const T *__restrict__ x, const T *__restrict__ xc,
                                                         const int32_t *__restrict__ agg, T scale, T *__restrict__ x_out,
                                                         const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i < n) x_out[i] = x[i] + scale * xc[agg[i]];
}

// one sweep on a CSR level, x_out != x; xc != nullptr: the sweep reads t_j = x_j + scale xc[agg[j]] (the prolongation folded in);
// TO: the type the result is stored as (double: level 0's last post-sweep of the single-precision cycle writes z)
template <class T, class TO, bool PROLONG>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_csr_sweep(MgCsrOf<T> A, const T *__restrict__ inv_d,
                                                           const T *__restrict__ b, const T *__restrict__ x,
                                                           const T *__restrict__ xc, const int32_t *__restrict__ agg,
                                                           T scale, TO *__restrict__ x_out, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    T s = 0;
    for (int k = A.row_ptrs[i]; k < A.row_ptrs[i + 1]; ++k) {
        const int j = A.cols[k];
        T t = x[j];
        if (PROLONG) t = t + scale * xc[agg[j]];
        s += A.vals[k] * t;
    }
    T ti = x[i];
    if (PROLONG) ti = ti + scale * xc[agg[i]];
    x_out[i] = (TO)(ti + (T)MG_OMEGA * ((b[i] - s) * inv_d[i]));
}

template <class T>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_csr_spmv(MgCsrOf<T> A, const T *__restrict__ x, T *__restrict__ y,
                                                          const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    T s = 0;
    for (int k = A.row_ptrs[i]; k < A.row_ptrs[i + 1]; ++k) s += A.vals[k] * x[A.cols[k]];
    y[i] = s;
}

// b_c[I] = sum over the members i of I, ascending, of r_i = b_i - (A x)_i; FROM: MG_FROM_AX the products come from `ax`,
// MG_FROM_RES the residuals themselves do (MgRestrictFrom, kernels.hpp)
template <class T, int FROM>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_restrict(int nc, const int32_t *__restrict__ agg_ptr,
                                                          const int32_t *__restrict__ agg_rows, MgCsrOf<T> A,
                                                          const T *__restrict__ b, const T *__restrict__ x,
                                                          const T *__restrict__ ax, T *__restrict__ bc,
                                                          const DevScalars *gate)
{
    MG_GATE();
    const int I = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (I >= nc) return;
    T acc = 0;
    for (int m = agg_ptr[I]; m < agg_ptr[I + 1]; ++m) {
        const int i = agg_rows[m];
        if (FROM == MG_FROM_RES) {
            acc += ax[i];
            continue;
        }
        T s;
        if (FROM == MG_FROM_AX) {
            s = ax[i];
        } else {
            s = 0;
            for (int k = A.row_ptrs[i]; k < A.row_ptrs[i + 1]; ++k) s += A.vals[k] * x[A.cols[k]];
        }
        acc += b[i] - s;
    }
    bc[I] = acc;
}

// coarsest level: unpreconditioned CG from x = 0 ([UPSTREAM] cg::initialize / step_1 / step_2, guards as k_cg_step1 / 2);
// TB: the type b arrives in (double under T = float: a hierarchy of one level, r = fl32(b))
template <class T, class TB>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_cg_init(int n, const TB *__restrict__ b, T *__restrict__ r,
                                                         T *__restrict__ x, T *__restrict__ p, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    r[i] = (T)b[i];
    x[i] = 0;
    p[i] = 0;
}

// the per-chunk partials of wide(a, b) = sum (double) a_i (double) b_i, as k_partials forms those of a dot product
__global__ __launch_bounds__(BLOCK) void k_mg_wide_dot(int n, const float *__restrict__ a, const float *__restrict__ b,
                                                       double *__restrict__ part, const DevScalars *gate)
{
    __shared__ double slot[N_WAVES];
    MG_GATE();
    const int chunk = blockIdx.x;
    const RowPair r = my_rows(chunk, n);
    double d = 0.0;
    if (r.n > 0) d += (double)a[r.row] * (double)b[r.row];
    if (r.n > 1) d += (double)a[r.row + 1] * (double)b[r.row + 1];
    const double s = block_sum(d, slot);
    if (threadIdx.x == 0) part[chunk] = s;
}

// the finaliser's tree over the chunk partials; what == 0: prev_rho <- rho (1 before the first), rho <- sum; 1: beta <- sum
__global__ __launch_bounds__(FIN_BLOCK) void k_mg_cg_fin(const double *part, int n_part, int what, int first, MgScalars *s,
                                                         const DevScalars *gate)
{
    __shared__ double slot[FIN_WAVES];
    MG_GATE();
    const double *const parts[2] = {part, part};
    double v[2];
    reduce_partials<1>(parts, n_part, slot, v);
    if (threadIdx.x != 0) return;
    if (what == 0) {
        s->prev_rho = first ? 1.0 : s->rho;
        s->rho = v[0];
    } else {
        s->beta = v[0];
    }
}

// (the quotients are formed in fp64 and rounded once to T)
template <class T>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_cg_step1(int n, T *__restrict__ p, const T *__restrict__ r,
                                                          const MgScalars *s, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double prev = s->prev_rho;
    const T tmp = (T)((prev == 0.0) ? 0.0 : s->rho / prev);
    p[i] = r[i] + tmp * p[i];
}

template <class T>
__global__ __launch_bounds__(MG_BLOCK) void k_mg_cg_step2(int n, T *__restrict__ x, T *__restrict__ r,
                                                          const T *__restrict__ p, const T *__restrict__ q,
                                                          const MgScalars *s, const DevScalars *gate)
{
    MG_GATE();
    const int i = blockIdx.x * MG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double beta = s->beta;
    if (beta == 0.0) return;
    const T t = (T)(s->rho / beta);
    x[i] += t * p[i];
    r[i] -= t * q[i];
}

// ------------------------------------------------------------------------------------------
// the tail: every level of at most mgTailRows rows in ONE workgroup -- down sweep, the coarsest CG, up sweep -- with a
// barrier between phases instead of a launch (those levels are bound by the dispatch latency of dependent launches, not by
// bytes).  The same operations in the same order as the kernels above, hence the same bits.
// ------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T tail_row_product(const MgTailLevelOf<T> &L, int i, const T *x, const T *xc, T scale)
{
    T s = 0;
    for (int k = L.row_ptrs[i]; k < L.row_ptrs[i + 1]; ++k) {
        const int j = L.cols[k];
        T t = x[j];
        if (xc) t = t + scale * xc[L.agg[j]];
        s += L.vals[k] * t;
    }
    return s;
}

// x_out = t + omega ((b - A t) inv_d), t = x (+ scale xc[agg]); x_out != x
template <class T>
__device__ __forceinline__ void tail_sweep(const MgTailLevelOf<T> &L, const T *b, const T *x, const T *xc, T scale, T *x_out)
{
    for (int i = threadIdx.x; i < L.n; i += BLOCK) {
        const T s = tail_row_product(L, i, x, xc, scale);
        T ti = x[i];
        if (xc) ti = ti + scale * xc[L.agg[i]];
        x_out[i] = ti + (T)MG_OMEGA * ((b[i] - s) * L.inv_d[i]);
    }
    __syncthreads();
}

__device__ __forceinline__ double2 tail_pair(const double *p, const RowPair &r) { return ld2(p, r); }
__device__ __forceinline__ double2 tail_pair(const float *p, const RowPair &r)
{
    double2 v;
    v.x = r.n > 0 ? (double)p[r.row] : 0.0;
    v.y = r.n > 1 ? (double)p[r.row + 1] : 0.0;
    return v;
}

// a . b (T = float: wide(a, b)) in the loop's tree: per-chunk partials as k_partials forms them, then the finaliser's tree
// (<= FIN_BLOCK chunks)
template <class T>
__device__ __forceinline__ double tail_dot(int n, const T *a, const T *b, double *part, double *lds)
{
    const int nc = (n + CHUNK_ROWS - 1) / CHUNK_ROWS;
    for (int c = 0; c < nc; ++c) {
        const RowPair r = my_rows(c, n);
        const double2 va = tail_pair(a, r), vb = tail_pair(b, r);
        double d = 0.0;
        if (r.n > 0) d += va.x * vb.x;
        if (r.n > 1) d += va.y * vb.y;
        const double s = block_sum(d, lds);
        if (threadIdx.x == 0) part[c] = s;
    }
    __syncthreads();
    double pv[2][FIN_VT], out[2];
    load_partials_as_finaliser<1>(part, nullptr, nc, pv);
    reduce_partials_as_finaliser<1>(pv, nc, lds, out);
    return out[0];
}

// The recursion of the cycle ("coarse visits") walked iteratively: `l` is the level being visited,
// `seen` holds, two bits per level, how many visits level l has had under the present visit of its parent (coarse_visits
// <= 3).  Both are the same in every thread, so every barrier is reached by the whole workgroup.  The first of the tail's
// levels is visited once per launch -- from nothing, or continued from the x_out of the launch before (T.continued); the
// levels below it coarse_visits times per visit of their parent, the coarsest once.
// A visit runs Tl.sweeps (keyword smootherSweeps) sweeps down and as many up.  x ping-pongs between the level's xa and xb so
// that no sweep writes the vector it reads: the first pre-sweep writes xa, so the last one leaves x in xa for an odd count
// and in xb for an even one; the post-sweeps go on alternating from there, which makes the last of them write xb (the
// tail's first level: x_out) whatever the count.  The count and the scale are the same in every thread.
template <class T>
__global__ __launch_bounds__(BLOCK) void k_mg_tail(MgTailOf<T> Tl, const T *b_in, T *x_out, const DevScalars *gate)
{
    __shared__ double lds[2 * FIN_WAVES];
    MG_GATE();
    const int last = Tl.count - 1;
    const int nu = Tl.sweeps;
    const T scale = (T)Tl.scale;
    uint32_t seen = 0;
    int l = 0;
    bool continued = Tl.continued != 0;
    for (;;) {
        if (l < last) {  // ---- down: the pre-sweeps, residual and restriction of one visit of level l ----
            const MgTailLevelOf<T> &L = Tl.lev[l];
            const T *b = l == 0 ? b_in : L.b;
            if (continued) {
                tail_sweep<T>(L, b, l == 0 ? x_out : L.xb, nullptr, scale, L.xa);
            } else {
                for (int i = threadIdx.x; i < L.n; i += BLOCK) L.xa[i] = (T)MG_OMEGA * (b[i] * L.inv_d[i]);
                __syncthreads();
            }
            const T *cur = L.xa;
            for (int k = 1; k < nu; ++k) {
                T *const next = cur == L.xa ? L.xb : L.xa;
                tail_sweep<T>(L, b, cur, nullptr, scale, next);
                cur = next;
            }
            T *bc = Tl.lev[l + 1].b;
            for (int I = threadIdx.x; I < L.n_coarse; I += BLOCK) {
                T acc = 0;
                for (int m = L.agg_ptr[I]; m < L.agg_ptr[I + 1]; ++m) {
                    const int i = L.agg_rows[m];
                    acc += b[i] - tail_row_product<T>(L, i, cur, nullptr, scale);
                }
                bc[I] = acc;
            }
            __syncthreads();
            ++l;  // (the first visit of the level below: from nothing)
            seen = (seen & ~(3u << (2 * l))) | (1u << (2 * l));
            continued = false;
            continue;
        }
        {  // ---- the coarsest solver ----
            const MgTailLevelOf<T> &L = Tl.lev[last];
            const T *b = last == 0 ? b_in : L.b;
            T *x = last == 0 ? x_out : L.xb;
            for (int i = threadIdx.x; i < L.n; i += BLOCK) {
                L.r[i] = b[i];
                x[i] = 0;
                L.p[i] = 0;
            }
            __syncthreads();
            double rho = 0.0;
            for (int it = 0; it < Tl.cg_iters; ++it) {
                const double prev = it == 0 ? 1.0 : rho;
                rho = tail_dot<T>(L.n, L.r, L.r, L.part, lds);
                const T tmp = (T)((prev == 0.0) ? 0.0 : rho / prev);
                for (int i = threadIdx.x; i < L.n; i += BLOCK) L.p[i] = L.r[i] + tmp * L.p[i];
                __syncthreads();
                for (int i = threadIdx.x; i < L.n; i += BLOCK) L.t[i] = tail_row_product<T>(L, i, L.p, nullptr, scale);
                __syncthreads();
                const double beta = tail_dot<T>(L.n, L.p, L.t, L.part, lds);
                if (beta != 0.0) {
                    const T t = (T)(rho / beta);
                    for (int i = threadIdx.x; i < L.n; i += BLOCK) {
                        x[i] += t * L.p[i];
                        L.r[i] -= t * L.t[i];
                    }
                }
                __syncthreads();
            }
        }
        // ---- up: the scaled correction and the post-sweeps, level by level, until a level is due another visit ----
        for (;;) {
            if (l == 0) return;
            --l;
            const MgTailLevelOf<T> &L = Tl.lev[l];
            const T *b = l == 0 ? b_in : L.b;
            const T *cur = (nu & 1) ? L.xa : L.xb;  // (what the last pre-sweep wrote)
            for (int k = 0; k < nu; ++k) {
                T *const next = k == nu - 1 ? (l == 0 ? x_out : L.xb) : (cur == L.xa ? L.xb : L.xa);
                tail_sweep<T>(L, b, cur, k == 0 ? Tl.lev[l + 1].xb : nullptr, scale, next);
                cur = next;
            }
            if (l == 0) return;
            const uint32_t had = (seen >> (2 * l)) & 3u;
            if ((int)had < Tl.coarse_visits) {  // (same b, continued from the level's xb)
                seen += 1u << (2 * l);
                continued = true;
                break;
            }
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
#define MG_LAUNCH(kernel, count, ...)                                                                    \
    do {                                                                                                 \
        if ((count) > 0) hipLaunchKernelGGL(kernel, dim3(mg_grid(count)), dim3(MG_BLOCK), 0, st, __VA_ARGS__); \
    } while (0)

void launch_mg_diag(hipStream_t st, const MgCsr &A, double *diag, double *inv_d) { MG_LAUNCH(k_mg_diag, A.n, A, diag, inv_d); }
void launch_mg_strongest(hipStream_t st, const MgCsr &A, const double *diag, const int32_t *agg, int want, bool hashed,
                         int32_t *s)
{
    if (hashed)
        MG_LAUNCH(k_mg_strongest<true>, A.n, A, diag, agg, want, s);
    else
        MG_LAUNCH(k_mg_strongest<false>, A.n, A, diag, agg, want, s);
}
void launch_mg_compose(hipStream_t st, int32_t n, const int32_t *cidx, int32_t *comp) { MG_LAUNCH(k_mg_compose, n, n, cidx, comp); }
void launch_mg_match(hipStream_t st, int32_t n, const int32_t *s, int32_t *agg, int32_t *left)
{
    MG_LAUNCH(k_mg_match, n, n, s, agg, left);
}
void launch_mg_join(hipStream_t st, int32_t n, const int32_t *s, int32_t *agg) { MG_LAUNCH(k_mg_join, n, n, s, agg); }
void launch_mg_root_flag(hipStream_t st, int32_t n, const int32_t *agg, int32_t *flag)
{
    MG_LAUNCH(k_mg_root_flag, n, n, agg, flag);
}
void launch_mg_coarse_index(hipStream_t st, int32_t n, const int32_t *agg, const int32_t *incl, int32_t *cidx, int32_t *rows)
{
    MG_LAUNCH(k_mg_coarse_index, n, n, agg, incl, cidx, rows);
}
void launch_mg_member_ptr(hipStream_t st, int32_t n, int32_t nc, const int32_t *sorted, int32_t *agg_ptr)
{
    MG_LAUNCH(k_mg_member_ptr, n, n, nc, sorted, agg_ptr);
}
void launch_mg_keys(hipStream_t st, const MgCsr &A, const int32_t *cidx, unsigned long long *keys)
{
    MG_LAUNCH(k_mg_keys, A.n, A, cidx, keys);
}
void launch_mg_head_flag(hipStream_t st, int32_t m, const unsigned long long *keys, int32_t *flag)
{
    MG_LAUNCH(k_mg_head_flag, m, m, keys, flag);
}
void launch_mg_compact(hipStream_t st, int32_t m, int32_t nc, const unsigned long long *keys, const double *vals,
                       const int32_t *pos, int32_t *row_ptrs, int32_t *cols, double *out)
{
    MG_LAUNCH(k_mg_compact, m, m, nc, keys, vals, pos, row_ptrs, cols, out);
}

void launch_mg_iota(hipStream_t st, int32_t m, int32_t *idx) { MG_LAUNCH(k_mg_iota, m, m, idx); }
void launch_mg_run_ptr(hipStream_t st, int32_t m, const int32_t *flag, const int32_t *pos, int32_t *ptr)
{
    MG_LAUNCH(k_mg_run_ptr, m, m, flag, pos, ptr);
}
void launch_mg_regalerkin(hipStream_t st, int32_t mc, const int32_t *ptr, const int32_t *src, const double *vals_in,
                          double *vals_out, bool stream)
{
    if (stream)
        MG_LAUNCH(k_mg_regalerkin<true>, mc, mc, ptr, src, vals_in, vals_out);
    else
        MG_LAUNCH(k_mg_regalerkin<false>, mc, mc, ptr, src, vals_in, vals_out);
}

size_t mg_temp_bytes(int32_t n, int32_t nnz)
{
    size_t a = 0, b = 0, c = 0, d = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, a, (const int32_t *)nullptr, (int32_t *)nullptr, std::max(n, nnz));
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                             (int32_t *)nullptr, n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, c, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const double *)nullptr, (double *)nullptr, nnz);
    // (mg_sort_entry_index: the same keys with the narrower payload)
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, d, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (const int32_t *)nullptr, (int32_t *)nullptr, nnz);
    return std::max(std::max(a, b), std::max(c, d)) + 256;
}
hipError_t mg_inclusive_sum(hipStream_t st, void *temp, size_t temp_bytes, const int32_t *in, int32_t *out, int32_t n)
{
    return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, n, st);
}
hipError_t mg_sort_rows(hipStream_t st, void *temp, size_t temp_bytes, const int32_t *keys, int32_t *keys_out,
                        const int32_t *rows, int32_t *rows_out, int32_t n)
{
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, rows, rows_out, n, 0, 32, st);
}
hipError_t mg_sort_entries(hipStream_t st, void *temp, size_t temp_bytes, const unsigned long long *keys,
                           unsigned long long *keys_out, const double *vals, double *vals_out, int32_t m)
{
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, vals, vals_out, m, 0, 64, st);
}
hipError_t mg_sort_entry_index(hipStream_t st, void *temp, size_t temp_bytes, const unsigned long long *keys,
                               unsigned long long *keys_out, const int32_t *idx, int32_t *idx_out, int32_t m)
{
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, idx, idx_out, m, 0, 64, st);
}

// ---- the cycle's kernels: one launcher per kernel template, instantiated for double and float below.  Only the kernel
//      instantiations the cycles use exist: what has none is refused by an assert ----
template <class T>
constexpr bool mg_is_float = std::is_same<T, float>::value;

template <class T>
void launch_mg_jacobi0(hipStream_t st, int32_t n, const T *b, const T *inv_d, T *x, const DevScalars *gate)
{
    MG_LAUNCH(k_mg_jacobi0<T>, n, n, b, inv_d, x, gate);
}
void launch_mg_sweep_epi(hipStream_t st, int32_t n, const double *b, const double *ax, const double *inv_d, const double *x,
                         double *x_out, const DevScalars *gate)
{
    MG_LAUNCH(k_mg_sweep_epi, n, n, b, ax, inv_d, x, x_out, gate);
}
template <class T>
void launch_mg_prolong(hipStream_t st, int32_t n, const T *x, const T *xc, const int32_t *agg, T scale, T *x_out,
                       const DevScalars *gate)
{
    MG_LAUNCH(k_mg_prolong<T>, n, n, x, xc, agg, scale, x_out, gate);
}
template <class T>
void launch_mg_csr_sweep(hipStream_t st, const MgCsrOf<T> &A, const T *inv_d, const T *b, const T *x, const T *xc,
                         const int32_t *agg, T scale, T *x_out, double *x_out64, const DevScalars *gate)
{
    if constexpr (mg_is_float<T>) {
        if (x_out64) {
            if (xc)
                MG_LAUNCH((k_mg_csr_sweep<float, double, true>), A.n, A, inv_d, b, x, xc, agg, scale, x_out64, gate);
            else
                MG_LAUNCH((k_mg_csr_sweep<float, double, false>), A.n, A, inv_d, b, x, xc, agg, scale, x_out64, gate);
            return;
        }
    }
    assert(!x_out64);
    if (xc)
        MG_LAUNCH((k_mg_csr_sweep<T, T, true>), A.n, A, inv_d, b, x, xc, agg, scale, x_out, gate);
    else
        MG_LAUNCH((k_mg_csr_sweep<T, T, false>), A.n, A, inv_d, b, x, xc, agg, scale, x_out, gate);
}
template <class T>
void launch_mg_csr_spmv(hipStream_t st, const MgCsrOf<T> &A, const T *x, T *y, const DevScalars *gate)
{
    MG_LAUNCH(k_mg_csr_spmv<T>, A.n, A, x, y, gate);
}
template <class T>
void launch_mg_restrict(hipStream_t st, int32_t nc, const int32_t *agg_ptr, const int32_t *agg_rows, const MgCsrOf<T> &A,
                        const T *b, const T *x, MgRestrictFrom from, const T *src, T *bc, const DevScalars *gate)
{
    // (what stands behind a product of the in-loop layout: A x in double precision, the residual in single precision)
    constexpr MgRestrictFrom behind = mg_is_float<T> ? MG_FROM_RES : MG_FROM_AX;
    assert(from == MG_FROM_A || from == behind);
    if (from == behind)
        MG_LAUNCH((k_mg_restrict<T, behind>), nc, nc, agg_ptr, agg_rows, A, b, x, src, bc, gate);
    else
        MG_LAUNCH((k_mg_restrict<T, MG_FROM_A>), nc, nc, agg_ptr, agg_rows, A, b, x, src, bc, gate);
}
template <class T>
void launch_mg_cg_init(hipStream_t st, int32_t n, const T *b, const double *b64, T *r, T *x, T *p, const DevScalars *gate)
{
    if constexpr (mg_is_float<T>) {
        if (b64) {
            MG_LAUNCH((k_mg_cg_init<float, double>), n, n, b64, r, x, p, gate);
            return;
        }
    }
    assert(!b64);
    MG_LAUNCH((k_mg_cg_init<T, T>), n, n, b, r, x, p, gate);
}
void launch_mg_cg_fin(hipStream_t st, const double *part, int32_t n_part, int what, int first, MgScalars *s,
                      const DevScalars *gate)
{
    hipLaunchKernelGGL(k_mg_cg_fin, dim3(1), dim3(FIN_BLOCK), 0, st, part, n_part, what, first, s, gate);
}
template <class T>
void launch_mg_cg_step1(hipStream_t st, int32_t n, T *p, const T *r, const MgScalars *s, const DevScalars *gate)
{
    MG_LAUNCH(k_mg_cg_step1<T>, n, n, p, r, s, gate);
}
template <class T>
void launch_mg_cg_step2(hipStream_t st, int32_t n, T *x, T *r, const T *p, const T *q, const MgScalars *s,
                        const DevScalars *gate)
{
    MG_LAUNCH(k_mg_cg_step2<T>, n, n, x, r, p, q, s, gate);
}
template <class T>
void launch_mg_tail(hipStream_t st, const MgTailOf<T> &Tl, const T *b, T *x, const DevScalars *gate)
{
    hipLaunchKernelGGL(k_mg_tail<T>, dim3(1), dim3(BLOCK), 0, st, Tl, b, x, gate);
}

#define MG_INSTANTIATE(T)                                                                                                      \
    template void launch_mg_jacobi0<T>(hipStream_t, int32_t, const T *, const T *, T *, const DevScalars *);                   \
    template void launch_mg_prolong<T>(hipStream_t, int32_t, const T *, const T *, const int32_t *, T, T *, const DevScalars *); \
    template void launch_mg_csr_sweep<T>(hipStream_t, const MgCsrOf<T> &, const T *, const T *, const T *, const T *,          \
                                         const int32_t *, T, T *, double *, const DevScalars *);                               \
    template void launch_mg_csr_spmv<T>(hipStream_t, const MgCsrOf<T> &, const T *, T *, const DevScalars *);                  \
    template void launch_mg_restrict<T>(hipStream_t, int32_t, const int32_t *, const int32_t *, const MgCsrOf<T> &, const T *, \
                                        const T *, MgRestrictFrom, const T *, T *, const DevScalars *);                        \
    template void launch_mg_cg_init<T>(hipStream_t, int32_t, const T *, const double *, T *, T *, T *, const DevScalars *);    \
    template void launch_mg_cg_step1<T>(hipStream_t, int32_t, T *, const T *, const MgScalars *, const DevScalars *);          \
    template void launch_mg_cg_step2<T>(hipStream_t, int32_t, T *, T *, const T *, const T *, const MgScalars *,               \
                                        const DevScalars *);                                                                   \
    template void launch_mg_tail<T>(hipStream_t, const MgTailOf<T> &, const T *, T *, const DevScalars *);
MG_INSTANTIATE(double)
MG_INSTANTIATE(float)
#undef MG_INSTANTIATE

// ---- what only the cycle in single precision launches ----
void launch_mg_twin(hipStream_t st, const MgCsr &A, const double *inv_d, float *vals32, float *inv_d32, int32_t *bad)
{
    MG_LAUNCH(k_mg_twin, A.n, A, inv_d, vals32, inv_d32, bad);
}
void launch_mg_jacobi0_in(hipStream_t st, int32_t n, const double *r, const float *inv_d, float *b, float *x,
                          const DevScalars *gate)
{
    MG_LAUNCH(k_mg_jacobi0_in, n, n, r, inv_d, b, x, gate);
}
void launch_mg_wide_dot(hipStream_t st, int32_t n, const float *a, const float *b, double *part, const DevScalars *gate)
{
    const int nc = (n + CHUNK_ROWS - 1) / CHUNK_ROWS;
    if (nc == 0) return;
    hipLaunchKernelGGL(k_mg_wide_dot, dim3(nc), dim3(BLOCK), 0, st, n, a, b, part, gate);
}
void launch_mg_widen(hipStream_t st, int32_t n, const float *x, double *out, const DevScalars *gate)
{
    MG_LAUNCH(k_mg_widen, n, n, x, out, gate);
}

}  // namespace ogl
