// sym_walk.hpp -- the row walk of the half storage of a banded symmetric matrix (SymLayout, host_matrix.hpp), once for
// every kernel that runs it and for both precisions (T = double: kernels_spmv_sym.hip; T = float, the fp32 twin of the
// planes: kernels_mixed.hip), and the host's one ladder over its instantiations (sym_dispatch).
//
// ND planes per chunk: plane j holds A(r, r + d[j]), d[0] = 0.  A lower entry A(r, r - d[j]) is read where its twin
// lives: plane j of row r - d[j] -- a coalesced strip of values that some workgroup reads (or has read) as upper
// entries, so DRAM delivers every coefficient once; the second reader finds it in L2 / the Infinity Cache.  8 ND + 1
// bytes per row instead of 8.1 per stored entry: measured 115 us against 139 us for the pattern-coded full storage on
// the 216^3 matrix (tools/sym_tune.hip, profiles/spmv_tune_r02.txt).  Rows are summed in ascending column order --
// furthest lower entry first, diagonal, upper entries -- so y and the fused dot partials have the same bits as
// k_spmv_sell / k_spmv_stream.
// FAST: d[1] == 1 and every further distance even (a box with an even line length) -- known at compile time, so the
// kernel stays straight-line code (a run-time test of the parity splits the loads into basic blocks that wait for each
// other: 130 us instead of 113, tools/sym_tune.hip var1/var2).  Then the two rows of a lane are an aligned pair in every
// strip: x and the lower values of the even distances come as one load per pair, the d = 1 neighbours from the diagonal
// pair and the lane's own plane-1 value.
// STREAM (double only; planes + vectors larger than the Infinity Cache): the planes that are read exactly once per launch
// are streamed past the caches -- the diagonal always, and with FAST also plane 1, whose second reader (the d = 1 lower
// entry of the next row) is the neighbouring lane: a lane shuffle instead of a load.
// Every load is issued whatever the mask says, at an index clamped into its array (mask -> gathers would be two round
// trips); the mask decides in sym_sum what is used.
#pragma once
#include <type_traits>

#include "device_common.hpp"

namespace ogl {

namespace {

struct SymOffsets {
    int d[SYM_MAX_OFFSETS];
};
// the distances of a layout as a kernel argument; *fast: the FAST instantiations serve it
inline SymOffsets sym_offsets(const DevSym &A, bool *fast)
{
    SymOffsets off;
    for (int j = 0; j < SYM_MAX_OFFSETS; ++j) off.d[j] = A.d[j];
    *fast = A.nd >= 2 && A.d[1] == 1;
    for (int j = 2; j < A.nd; ++j) *fast = *fast && (A.d[j] % 2 == 0);
    return off;
}
// f(off, ND, FAST, STREAM) with the three as std::integral_constant: the instantiation that serves A (STREAM: A.stream;
// a caller whose kernel has no such parameter ignores it)
template <class F>
inline void sym_dispatch(const DevSym &A, F &&f)
{
    bool fast;
    const SymOffsets off = sym_offsets(A, &fast);
    auto with_nd = [&](auto nd) {
        if (fast && A.stream)
            f(off, nd, std::true_type{}, std::true_type{});
        else if (fast)
            f(off, nd, std::true_type{}, std::false_type{});
        else if (A.stream)
            f(off, nd, std::false_type{}, std::true_type{});
        else
            f(off, nd, std::false_type{}, std::false_type{});
    };
    static_assert(SYM_MAX_OFFSETS == 4, "ND = 2, 3, 4 below");
    if (A.nd == 2)
        with_nd(std::integral_constant<int, 2>{});
    else if (A.nd == 3)
        with_nd(std::integral_constant<int, 3>{});
    else
        with_nd(std::integral_constant<int, 4>{});
}

// own planes: diagonal and upper entries of the lane's two rows
template <class T, int ND, bool FAST, bool STREAM>
__device__ __forceinline__ void sym_own_planes(typename PairOf<T>::type (&up)[ND], int chunk, const T *__restrict__ planes)
{
    using P = typename PairOf<T>::type;
    static_assert(!STREAM || std::is_same<T, double>::value, "no non-temporal float loads");
    const T *own = planes + (long)chunk * (ND * CHUNK_ROWS) + threadIdx.x * ROWS_PER_THREAD;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        if constexpr (STREAM)
            up[j] = (j == 0 || (FAST && j == 1)) ? ld_pair_stream(own + (long)j * CHUNK_ROWS)
                                                 : *reinterpret_cast<const P *>(own + (long)j * CHUNK_ROWS);
        else
            up[j] = *reinterpret_cast<const P *>(own + (long)j * CHUNK_ROWS);
    }
}
// the twins of the lower entries: plane j at rows row - d[j], row + 1 - d[j]
template <class T, int ND, bool FAST, bool STREAM>
__device__ __forceinline__ void sym_twin_planes(typename PairOf<T>::type (&lo)[ND], const typename PairOf<T>::type (&up)[ND],
                                                int row, const SymOffsets &off, const T *__restrict__ planes)
{
    using P = typename PairOf<T>::type;
#pragma unroll
    for (int j = 1; j < ND; ++j) {
        const int r0 = max(row - off.d[j], 0), r1 = max(row + 1 - off.d[j], 0);
        const long a0 = (long)(r0 >> 9) * (ND * CHUNK_ROWS) + (long)j * CHUNK_ROWS + (r0 & (CHUNK_ROWS - 1));
        const long a1 = (long)(r1 >> 9) * (ND * CHUNK_ROWS) + (long)j * CHUNK_ROWS + (r1 & (CHUNK_ROWS - 1));
        if (FAST && j >= 2) {  // even distance: rows r0, r0 + 1 are an aligned pair of one chunk's plane
            lo[j] = *reinterpret_cast<const P *>(planes + a0);
        } else if (FAST) {     // d = 1: A(row + 1, row) is this lane's own upper entry of row
            if (STREAM) {      // A(row, row - 1) is the previous lane's second plane-1 value (lane 0: from memory)
                lo[j].x = __shfl_up(up[1].y, 1, WAVE);
                if ((threadIdx.x & (WAVE - 1)) == 0) lo[j].x = planes[a0];
            } else {
                lo[j].x = planes[a0];
            }
            lo[j].y = up[1].x;
        } else {
            lo[j].x = planes[a0];
            lo[j].y = planes[a1];
        }
    }
    static_assert(CHUNK_ROWS == 512, "row >> 9 above");
}
// a vector at the columns of the two rows' entries; vd: the vector at the rows themselves (ld2)
template <class T, int ND, bool FAST>
__device__ __forceinline__ void sym_gather(typename PairOf<T>::type (&vl)[ND], typename PairOf<T>::type (&vu)[ND],
                                           const typename PairOf<T>::type &vd, int row, int n_rows, const SymOffsets &off,
                                           const T *__restrict__ v)
{
    using P = typename PairOf<T>::type;
    const int last = n_rows - 1, last_pair = last & ~1;  // (a pair load at the last even row: the vectors are allocated two past n_rows)
#pragma unroll
    for (int j = 1; j < ND; ++j) {
        if (FAST && j >= 2) {
            vl[j] = *reinterpret_cast<const P *>(v + min(max(row - off.d[j], 0), last_pair));
            vu[j] = *reinterpret_cast<const P *>(v + min(row + off.d[j], last_pair));
        } else if (FAST) {     // the neighbours of a pair at distance 1: the pair itself + one on each side
            vl[j].x = v[min(max(row - 1, 0), last)];
            vl[j].y = vd.x;
            vu[j].x = vd.y;
            vu[j].y = v[min(row + 2, last)];
        } else {
            vl[j].x = v[min(max(row - off.d[j], 0), last)];
            vl[j].y = v[min(max(row + 1 - off.d[j], 0), last)];
            vu[j].x = v[min(row + off.d[j], last)];
            vu[j].y = v[min(row + 1 + off.d[j], last)];
        }
    }
}
// The two row sums on top of acc, in ascending column order: the furthest lower entry first, the diagonal, the upper
// entries; every product rounds, then is added (SPMV_RESIDUAL: subtracted).  m0, m1: which of the 2 ND - 1 entries the
// two rows have: bit (ND-1-j) = the one at -d[j], bit (ND-1+j) = at +d[j]
template <int MODE, class T, int ND>
__device__ __forceinline__ typename PairOf<T>::type sym_sum(
    unsigned m0, unsigned m1, const typename PairOf<T>::type (&up)[ND], const typename PairOf<T>::type (&lo)[ND],
    const typename PairOf<T>::type &xd, const typename PairOf<T>::type (&xl)[ND], const typename PairOf<T>::type (&xu)[ND],
    typename PairOf<T>::type acc)
{
    auto add = [](unsigned m, int bit, T &a, T c, T v) {
        if ((m >> bit) & 1u) {
            const T p = c * v;
            a = (MODE == SPMV_RESIDUAL) ? a - p : a + p;
        }
    };
#pragma unroll
    for (int j = ND - 1; j >= 1; --j) {
        add(m0, ND - 1 - j, acc.x, lo[j].x, xl[j].x);
        add(m1, ND - 1 - j, acc.y, lo[j].y, xl[j].y);
    }
    add(m0, ND - 1, acc.x, up[0].x, xd.x);
    add(m1, ND - 1, acc.y, up[0].y, xd.y);
#pragma unroll
    for (int j = 1; j < ND; ++j) {
        add(m0, ND - 1 + j, acc.x, up[j].x, xu[j].x);
        add(m1, ND - 1 + j, acc.y, up[j].y, xu[j].y);
    }
    return acc;
}

// The rows of one chunk -- every load, the mask, the sums -- of k_spmv_sym, phase S of the held-q turn and k_mx_spmv_sym.
// Returns the pair's sums (SPMV_RESIDUAL: b - A x); xd_out: x at the two rows themselves.
template <int MODE, class T, int ND, bool FAST, bool STREAM>
__device__ __forceinline__ typename PairOf<T>::type sym_rows(int chunk, const RowPair &rp, int n_rows, const SymOffsets &off,
                                                             const uint8_t *__restrict__ mask, const T *__restrict__ planes,
                                                             const T *__restrict__ x, const T *__restrict__ b,
                                                             typename PairOf<T>::type &xd_out)
{
    using P = typename PairOf<T>::type;
    const unsigned mm = *reinterpret_cast<const unsigned short *>(mask + rp.row);
    const unsigned m0 = mm & 0xffu, m1 = mm >> 8;
    P acc;
    acc.x = acc.y = T(0);
    if (MODE == SPMV_RESIDUAL) acc = ld2(b, rp);
    P up[ND], lo[ND], xl[ND], xu[ND];
    sym_own_planes<T, ND, FAST, STREAM>(up, chunk, planes);
    const P xd = xd_out = ld2(x, rp);
    sym_twin_planes<T, ND, FAST, STREAM>(lo, up, rp.row, off, planes);
    sym_gather<T, ND, FAST>(xl, xu, xd, rp.row, n_rows, off, x);
    return sym_sum<MODE, T, ND>(m0, m1, up, lo, xd, xl, xu, acc);
}

}  // namespace

}  // namespace ogl
