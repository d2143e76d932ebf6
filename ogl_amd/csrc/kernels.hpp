// kernels.hpp -- launchers of the hand-written gfx950 kernels (kernels_*.hip; what they share: device_common.hpp).
// Everything the Krylov loop of the reference delegates to Ginkgo.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace ogl {

// OpenFOAMDistStoppingCriterion parameters (StoppingCriterion.H:32-72)
struct DevCriterion {
    double tolerance, rel_tol;
    int32_t min_iter, max_iter, frequency, export_res;
};

// Solver scalars and criterion state, resident in device memory for the whole solve so that the
// loop never synchronises with the host (the reference syncs D2H on every evaluated check,
// StoppingCriterion.C:95-97).
struct DevScalars {
    double rho, prev_rho, beta;         // CG  ([UPSTREAM] gko::solver::Cg scalars)
    double alpha, omega, gamma;         // BiCGStab extras
    double norm_factor;                 // StoppingCriterion.H:136
    double init_res, res;               // init_normalised_res_norm_, normalised_res_norm_
    double xbar;                        // mean(x) for the norm factor (StoppingCriterion.C:17-19)
    double sums[4];                     // rank-local sums staged for the all-reduce
    int32_t iter;                       // iter_ : number of check_impl calls so far
    int32_t stop;                       // criterion said stop; later kernels become no-ops
    int32_t n_evals;                    // checks that evaluated the norm
    int32_t stop_phase;                 // BiCGStab: 1 = stopped at the mid-step check (finalize x)
    int32_t stop_turn;                  // BiCGStab: turn index of that stop
    int32_t comm_error;                 // peer all-reduce timed out (a rank is gone): solve fails
    double stale_norm;                  // GMRES: sum|r| of the last restart (what the criterion sees)
    DevCriterion crit;                  // this solve's criterion (kernel arguments stay solve-independent)
    int32_t x_pending;                  // GKOCG: step_2r's x update is still to be applied by a step_1x
    // GKOCG with x touched every K-th turn (PRing): bit i of defer_valid = the head of ring position i left
    // t_ring[i] * (its old p, still intact in ring buffer i) pending
    int32_t defer_valid;
    double t_ring[8];
    // Where a multi-rank turn waits (per solve; wall_clock64 ticks of 10 ns): halo_wait_ticks = sum over the workgroups
    // that waited for the neighbours' puts of the longest of their flag waits (halo_waits of them: boundary workgroups
    // of the SpMV, or the single waiter of peerSafeWait / the separate finish kernel); reduce_wait_ticks = sum over
    // the in-finaliser all-reduces of the longest mailbox wait (reduce_waits of them).  bench.py reports both per turn
    // and rank, so that a scaling curve below DESIGN.md section 6's table can be attributed.
    uint32_t halo_waits;
    unsigned long long halo_wait_ticks, reduce_wait_ticks;
    uint32_t reduce_waits;
    uint32_t launch_seq;  // leader finalisation (LeadBox): tag of the next leader launch's mailbox words
    // IC / ILU / IRILU: the factor's breakdown word (FactorPart::breakdown), Chebyshev: its table's (ChebTable::breakdown),
    // copied here after the last kernel of the solve so that it comes back with the final scalars
    int32_t factor_breakdown;
    int32_t pad_;
};

// GKOCG, three-launch leader turn: K search-direction buffers used in turn (the head of turn j reads b[j % K] and writes
// b[(j + 1) % K]), so that x is read and written by every K-th head only (k_cg_step1x_fin).  k == 0: p in place, x every turn.
constexpr int P_RING_MAX = 8;
struct PRing {
    double *b[P_RING_MAX] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t k = 0;      // 0 | 2 | 4 | 8
    int32_t phase = 0;  // turn % k of the head this is handed to
};

// Persistent device CSR ("<field>_matrix", CsrMatrixWrapper.H:163-210) + halo part.
struct DevCsr {
    int32_t n_rows = 0;
    int32_t nnz = 0;
    const int32_t *row_ptrs = nullptr;  // [n_rows + 1]
    const int32_t *cols = nullptr;      // [nnz + NNZ_PAD]
    const double *vals = nullptr;       // [nnz + NNZ_PAD]
    // the matrix does not fit the Infinity Cache next to the solver's vectors: its values and columns are
    // streamed past the caches (non-temporal loads); a matrix that fits stays cached from turn to turn
    bool stream = false;
    // consecutive chunks one XCD takes before the next XCD's group starts (0: the built-in 4).  Large groups
    // (slabs of tens of thousands of rows) keep the x window of an irregular pattern in ONE L2
    int32_t xcd_group = 0;
    // packed columns (Stream21Chunk, common.hpp): when set, the kernel reads these instead of `cols`
    const Stream21Chunk *chunks21 = nullptr;
    const uint4 *codes21 = nullptr;
    const int32_t *far_idx21 = nullptr, *far_col21 = nullptr;  // the chunks' far entries (Stream21Chunk::far_off / far_n)
    // banded patterns: the order in which the workgroups take the chunks (band_block_order, host_matrix.hpp: the
    // chunks of rows r and r +- band on one XCD; -1 = no chunk), n_blocks entries; nullptr = the XCD groups above
    const int32_t *block_order = nullptr;
    int32_t n_blocks = 0;
    // CSR-stream kernel: rounds in which a pass's 4096 products go through LDS (2: half the LDS, six workgroups per CU
    // instead of four -- measured 199 against 196 us at 216^3: the kernel does not wait for wavefronts; property spmvLdsRounds)
    int32_t lds_rounds = 1;
};

// Rows that own non-local entries, for "y += A_non_local * recv" (distributed::Matrix::apply).
struct DevHalo {
    int32_t n_boundary_rows = 0;            // distinct rows with non-local entries
    const int32_t *boundary_rows = nullptr; // [n_boundary_rows]
    const int32_t *entry_ptrs = nullptr;    // [n_boundary_rows + 1] into cols/vals
    const int32_t *cols = nullptr;          // position in the receive buffer
    const double *vals = nullptr;           // -bouCoeffs, row-sorted (HostMatrix.C:708-732)
    int32_t n_send = 0;
    const int32_t *send_idxs = nullptr;     // rows gathered into the send buffer
};

// Mailbox of the leader finalisation (device_common.hpp): a few 8-byte words in fine-grained (uncached) device memory,
// written by workgroup 0 of a launch and polled by the others.  box == nullptr: every workgroup reduces the partials
// itself (small systems) -- or the finalisers are launches of their own.
struct LeadBox {
    unsigned long long *box = nullptr;
    long long timeout_ticks = 0;  // wall_clock64 ticks (10 ns) a polling workgroup waits before it gives the solve up
    int32_t early_loads = 0;      // 1: a polling workgroup asks for its rows before it polls (else after)
};
constexpr int LEAD_BOX_WORDS = 96;  // 16 wavefront sums x up to 3 arrays x 2 half-words
constexpr int LEAD_REPLICAS = 16;   // copies of the mailbox (workgroup b polls copy b % 16), LEAD_REPLICA_STRIDE words apart
constexpr int LEAD_REPLICA_STRIDE = 544;  // 4352 bytes: 4 KiB + 256, so that the copies fall into different channels

enum SpmvMode { SPMV_PLAIN = 0, SPMV_RESIDUAL = 1 };

// y = A x (PLAIN) or y = b - A x (RESIDUAL: accumulator starts at b_i and subtracts the products
// in stored order, which is what Ginkgo's advanced apply with alpha=-1, beta=1 evaluates).
// dots.part != nullptr: also one partial of sum_i w_i*y_i (and y_i*y_i) per chunk of CHUNK_ROWS rows.
// `gate` (may be nullptr): kernel returns immediately when gate->stop is set.
// (T = float: the inner product of the mixed mode, whose partials are sums of products of the float64 casts)
template <class T>
struct SpmvDotsOf {
    const T *with = nullptr;    // w in sum_i w_i*y_i (CG: x itself; BiCGStab: rr or s)
    double *part = nullptr;     // per-chunk partials of w.y, or nullptr
    double *part_yy = nullptr;  // per-chunk partials of y.y (needs `part`), or nullptr
};
using SpmvDots = SpmvDotsOf<double>;
// What a waiter for halo exchange number `seq` needs (peer-put transport; PeerHalo below): lane i of a waiting workgroup
// reads local_flag[i] until it carries `seq`, for at most timeout_ticks of the 100 MHz wall clock.
struct HaloWait {
    const unsigned long long *local_flag = nullptr;  // this rank's flags, one per neighbour
    int32_t n_neigh = 0;
    uint32_t seq = 0;
    long long timeout_ticks = 0;
};
// Non-local part of the product inside the LOCAL kernel (peer-put transport): the workgroup of a chunk that
// holds boundary rows waits for the neighbours' flags of this SpMV, then continues the accumulators of its
// boundary rows over their non-local entries in stored order -- local first, then non-local, as
// distributed::Matrix::apply does -- before y and the fused dot partials are formed.  chunk_bptr == nullptr: none.
struct HaloFused {
    const int32_t *chunk_bptr = nullptr;     // [n_chunks + 1] ranges of boundary_rows per chunk
    const int32_t *boundary_rows = nullptr;  // as DevHalo
    const int32_t *entry_ptrs = nullptr;
    const int32_t *cols = nullptr;
    const double *vals = nullptr;
    const double *recv = nullptr;            // this SpMV's receive block
    HaloWait wait;
    DevScalars *s = nullptr;                 // receives comm_error / stop when a neighbour does not show up
};
void launch_spmv(hipStream_t st, const DevCsr &A, int mode, const double *x, const double *b,
                 double *y, const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf = HaloFused{});

// matrixFormat Ell (CsrMatrixWrapper.H:146-149): `width` slots per row, slot-major (column-major in
// Ginkgo's terms) with leading dimension `stride` >= n_rows; padding slots carry column -1 and are
// skipped, so a row is summed in the same stored order as in the CSR kernel (bit-identical y).
struct DevEll {
    int32_t n_rows = 0;
    int32_t width = 0;
    int64_t stride = 0;
    const int32_t *cols = nullptr;  // [width * stride]
    const double *vals = nullptr;   // [width * stride]
    bool stream = false;            // as DevCsr::stream
};
void launch_spmv_ell(hipStream_t st, const DevEll &A, int mode, const double *x, const double *b,
                     double *y, const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf = HaloFused{});
// Index-compressed chunked ELL (SellChunk, common.hpp), device view.
struct DevSell {
    int32_t n_rows = 0;
    const SellChunk *chunks = nullptr;  // [n_chunks]
    const int32_t *dict = nullptr;      // column - row offsets, ascending per chunk
    const uint8_t *codes = nullptr;     // thread-major: [thread][slot][row of the pair]
    const double *vals = nullptr;
    // spill (nullptr: none): tails of the rows longer than their chunk's cap, added by the chunk's
    // workgroup after the planes.  spill_chunk_ptr[c] .. [c + 1] = this chunk's range of spill_rows;
    // spill_ptrs = their entry ranges in spill_cols / spill_vals
    const int32_t *spill_chunk_ptr = nullptr, *spill_rows = nullptr, *spill_ptrs = nullptr, *spill_cols = nullptr;
    const double *spill_vals = nullptr;
    bool stream = false;  // as DevCsr::stream, for the value planes and the 16 / 32-bit code words
    int32_t xcd_group = 0;  // as DevCsr::xcd_group
    // rows of a wavefront's window stored in an order of their own (longest first: SellDev::build, sort_windows):
    // rmap[chunk * CHUNK_ROWS + slot row] = the row of the chunk whose entries the slot row holds.  The workgroup
    // hands the sums back to the rows' owners through LDS before y and the dot partials are formed, so y, the
    // per-row order of the products and the partials are those of the plain layout.  PLAIN mode, no spill, no halo.
    const uint16_t *rmap = nullptr;
    const int32_t *block_order = nullptr;  // as DevCsr::block_order
    int32_t n_blocks = 0;
};
void launch_spmv_sell(hipStream_t st, const DevSell &A, int mode, const double *x, const double *b,
                      double *y, const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf = HaloFused{});
// Half storage of a symmetric matrix on a banded pattern (SymLayout, host_matrix.hpp), device view.
struct DevSym {
    int32_t n_rows = 0;
    int32_t nd = 0;                 // planes per chunk: diagonal + distances
    int32_t d[4] = {0, 0, 0, 0};    // the distances, ascending, d[0] = 0
    const uint8_t *mask = nullptr;  // [n_chunks * CHUNK_ROWS] which entries a row has
    const double *planes = nullptr; // [n_chunks][nd][CHUNK_ROWS]
    bool stream = false;            // as DevCsr::stream, for the planes that are read once per launch
    // workgroup b takes chunk block_order[b] (-1: none), n_blocks workgroups (band_block_order); nullptr: default map
    const int32_t *block_order = nullptr;
    int32_t n_blocks = 0;
};
void launch_spmv_sym(hipStream_t st, const DevSym &A, int mode, const double *x, const double *b, double *y,
                     const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf = HaloFused{});
// Half storage with per-chunk distances and explicit exceptions (SymxChunk, common.hpp), device view.
struct DevSymx {
    int32_t n_rows = 0;
    // headers in dispatch order (symx_block_order): workgroup b works on chunks[b].chunk.  Two lists: the chunks the
    // lean kernel takes (no explicit entries or simple ones) and the ones the general kernel takes
    const SymxChunk *chunks = nullptr, *chunks_general = nullptr;
    int32_t n_blocks_general = 0;
    const uint8_t *mask = nullptr;      // [n_chunks * CHUNK_ROWS]
    const double *planes = nullptr;
    const int32_t *ex_rowptr = nullptr, *ex_cols = nullptr;  // explicit entries (per-chunk row pointers, columns)
    const int32_t *ex_lrow = nullptr;                        // ... their rows within the chunk | SYMX_BEHIND_BIT
    const double *ex_vals = nullptr;
    bool stream = false;
    bool fast = false;  // every chunk: first distance 1, further distances even (pair-load instantiation)
    int32_t xcd_group = 0;
    int32_t n_blocks = 0;
};
void launch_spmv_symx(hipStream_t st, const DevSymx &A, int mode, const double *x, const double *b, double *y,
                      const SpmvDots &dots, const DevScalars *gate, const HaloFused &hf = HaloFused{});
// out[i] = map[i] >= 0 ? source[map[i]] : 0   (coefficient permutation into the padded ELL slots)
void launch_gather_coeffs_masked(hipStream_t st, int64_t n, const int32_t *map, const double *source,
                                 double *out);
// the same into the value planes of a chunked layout (SellChunk), one workgroup per chunk
void launch_gather_sell(hipStream_t st, int32_t n_chunks, const SellChunk *chunks, const int32_t *map,
                        const double *source, double *out);

// coeffs[i] = source[ldu_mapping[i]]   (row_gather, HostMatrix.C:700-703)
void launch_gather_coeffs(hipStream_t st, int32_t nnz, const int32_t *ldu_mapping,
                          const double *source, double *coeffs);
// inv_diag[i] = 1 / A(i,i)   (Jacobi generate with max_block_size 1)
void launch_jacobi_generate(hipStream_t st, const DevCsr &A, double *inv_diag);
// the same with diag_pos[i] = position of row i's first diagonal entry (-1: none), found once per pattern
void launch_jacobi_generate_pos(hipStream_t st, const DevCsr &A, const int32_t *diag_pos, double *inv_diag);
// ... from a contiguous copy of the diagonal in device-row order (the staged lduMatrix source)
void launch_jacobi_generate_diag(hipStream_t st, int32_t n_rows, const double *diag, double *inv_diag);

// Block Jacobi with maxBlockSize k > 1 (Preconditioner.H:91-105): inverted diagonal blocks,
// row-major, `stride` x `stride` doubles per block.
struct DevBlockJacobi {
    int32_t n_rows = 0;
    int32_t n_blocks = 0;
    int32_t stride = 0;                  // = maxBlockSize
    const int32_t *block_ptrs = nullptr; // [n_blocks + 1] first row of each block
    const int32_t *row_block = nullptr;  // [n_rows] block of each row
    double *blocks = nullptr;            // [n_blocks * stride * stride]
    // every block but the last holds exactly `stride` rows (what agglomeration gives on a mesh without
    // repeated row patterns): block and first row follow from the row index, no index loads in the apply
    int32_t uniform = 0;
    // renumbered device copy: the blocks are those of the CALLER's numbering (Preconditioner.H:91-105 generates on
    // the matrix OpenFOAM hands over) -- block_ptrs / row_block refer to positions there, rows[position] = device
    // row, pos[device row] = position.  nullptr: the device copy is in the caller's numbering.
    const int32_t *rows = nullptr, *pos = nullptr;
    // ... and the block rows are stored at their device rows (rows[position] * stride; the direct apply) instead of
    // block-major in the caller's order (the staged apply)
    int32_t by_device_row = 0;
    // k_bj_apply_perm: consecutive 512-position ranges one XCD takes (0: chosen from the size, 4 .. 256)
    int32_t perm_xcd_group = 0;
};
constexpr int MAX_JACOBI_BLOCK = 32;
// blocks[b] = inverse of A(block b, block b) by Gauss-Jordan with partial pivoting
void launch_bj_generate(hipStream_t st, const DevCsr &A, const DevBlockJacobi &J,
                        bool group_lanes = true);  // blocks of <= 8 rows: 4 | 8 lanes per block instead of a thread
// out = M^-1 in : per row, the block row times the block's slice of `in`, summed left to right;
// dot_part != nullptr: also the per-chunk partials of sum_i in_i * out_i
void launch_bj_apply(hipStream_t st, const DevBlockJacobi &J, const double *in, double *out,
                     double *dot_part, const DevScalars *gate);
// the same through a permutation in three launches (J.rows / J.pos set, blocks block-major in the caller's order):
// in -> caller's order (one gather per row), contiguous apply, back to the device order + the dot partials.
// tmp_in / tmp_out: two scratch vectors of n_rows doubles
void launch_bj_apply_staged(hipStream_t st, const DevBlockJacobi &J, const double *in, double *out, double *dot_part,
                            const DevScalars *gate, double *tmp_in, double *tmp_out);

// ISAI / GISAI (Preconditioner.H:225-258): row i of the approximate inverse W lives on the pattern J of
// row i of S^sparsityPower (S = tril(A) resp. A, built on the host) and solves a dense system over it by
// Gaussian elimination with partial pivoting.  spd: A(J,J) y = e_i, W(i,J) = y / sqrt(y_i); general:
// A(J,J)^T y = e_i, W(i,J) = y.  Rows of up to ISAI_THREAD_ROW entries: one thread per row (per-thread
// arrays); longer ones, up to MAX_ISAI_ROW: one wavefront per row, the system in LDS, lane = column --
// the same operations on every element in the same order, so both give the oracle's bits.
// Rows beyond MAX_ISAI_ROW, up to MAX_ISAI_HUGE_ROW (2048: the square of a polyhedral mesh's pattern): one WORKGROUP per row, the system in global scratch
// (bs x bs doubles per row), the same elimination, the back substitution column by column (the oracle's
// solve_dense_wide: a row-wise walk would be one dependent chain of bs^2 / 2 operations).  [UPSTREAM] Ginkgo solves
// rows beyond its in-kernel limit through an iterative "excess system" (GMRES to 1e-6): an approximation of this.
constexpr int ISAI_THREAD_ROW = 32;
constexpr int MAX_ISAI_ROW = 64;
constexpr int MAX_ISAI_HUGE_ROW = 2048;
// max_row = longest row of W (selects the per-thread scratch size: 8, 16 or 32);
// wide_rows[n_wide] = the rows with ISAI_THREAD_ROW < entries <= MAX_ISAI_ROW
void launch_isai_generate(hipStream_t st, const DevCsr &A, int spd, const int32_t *w_row_ptrs,
                          const int32_t *w_cols, double *w_vals, int32_t max_row,
                          const int32_t *wide_rows, int32_t n_wide,
                          bool group_lanes = true);  // rows of <= 8 entries: 4 | 8 lanes per row instead of a thread
// huge_rows[first .. first + count): rows wider than MAX_ISAI_ROW; scratch_off[k] = where row huge_rows[k]'s
// system starts in `scratch` (doubles)
void launch_isai_generate_huge(hipStream_t st, const DevCsr &A, int spd, const int32_t *w_row_ptrs,
                               const int32_t *w_cols, double *w_vals, const int32_t *huge_rows,
                               const int64_t *scratch_off, int32_t first, int32_t count, double *scratch);

// Incomplete factorisations (kernels_factor.hip; preconditioners IC, ILU, IRILU).  The factor lives in the caller's
// numbering (FactorStructure, host_matrix.hpp): one CSR `f` (ILU: strict L, the diagonal, U; IC: L with the diagonal
// last), diag[i] = position of (i, i).  Level-scheduled kernels take one thread per row of a level; a run of thin levels
// goes to one workgroup that walks them with a barrier between levels (no waits between workgroups).
struct DevFactor {
    int32_t n_rows = 0;
    int32_t ic = 0;
    const int32_t *row_ptrs = nullptr, *cols = nullptr, *diag = nullptr;
    double *vals = nullptr;
    // update lists per strictly lower entry (FactorStructure::upd_*)
    const int32_t *upd_ptr = nullptr, *upd_a = nullptr, *upd_b = nullptr;
    int32_t *breakdown = nullptr;  // atomicMin of the rows with a zero (ILU) / non-positive (IC) pivot
};
// one triangle of the factor, row by row: lower: off-diagonal entries [beg[i], end[i]), the diagonal at end[i] (unit:
// none); upper: the diagonal at beg[i], off-diagonal entries (beg[i], end[i])
struct DevTri {
    const int32_t *beg = nullptr, *end = nullptr, *cols = nullptr;
    const double *vals = nullptr;
    int32_t upper = 0, unit = 0;
};
// f[e] = sum of src[map[map_ptr[e] .. map_ptr[e + 1])] in that order
void launch_factor_gather(hipStream_t st, int32_t nf, const int32_t *map_ptr, const int32_t *map, const double *src,
                          double *f);
// IC(0) / ILU(0) of the rows of levels [l0, l1) (seg: thin = one workgroup walks them)
// (level_ptr: the same array on the host and on the device)
void launch_factor_levels(hipStream_t st, const DevFactor &F, const int32_t *level_ptr_host, const int32_t *level_ptr,
                          const int32_t *level_rows, int32_t l0, int32_t l1, bool thin);
// x = T^-1 b on the rows of levels [l0, l1); b_perm != nullptr: b_i = b[b_perm[i]].  x may be b (in place).
void launch_tri_levels(hipStream_t st, const DevTri &T, const int32_t *level_ptr_host, const int32_t *level_ptr,
                       const int32_t *level_rows, int32_t l0, int32_t l1, bool thin, const double *b, const int32_t *b_perm, double *x,
                       const DevScalars *gate);
// IRILU: sweeps per triangle ([UPSTREAM] Ir with BJ(1), 5 iterations, Preconditioner.H:147-178)
constexpr int IRILU_SWEEPS = 5;
// one Richardson sweep x_out = x + D^-1 (b - T x) over all rows (inv_d == nullptr: D = I)
void launch_tri_sweep(hipStream_t st, int32_t n, const DevTri &T, const double *inv_d, const double *b,
                      const double *x, double *x_out, const DevScalars *gate);
// Keyword factorSweeps: the factor from synchronous fixed-point sweeps, one thread per row, every
// entry from the values the sweep before left (`in` -> `out`, never in place).  a: the gathered values of A on the
// factor's pattern.  gs_*: ILU's update pairs in gather form (build_factor_gather_lists); IC reads F.upd_*.
// start: l_ii = sqrt(a_ii), l_ij = a_ij / sqrt(a_jj) (IC); l_ij = a_ij / a_jj, u_ij = a_ij (ILU).
void launch_factor_sweep_start(hipStream_t st, const DevFactor &F, const double *a, double *out);
// judge: the last sweep -- the smallest row whose l_ii is not > 0 (IC) / whose u_ii is 0 or not finite (ILU) goes into
// F.breakdown
void launch_factor_sweep(hipStream_t st, const DevFactor &F, const int32_t *gs_ptr, const int32_t *gs_a,
                         const int32_t *gs_b, const double *a, const double *in, double *out, bool judge);
// Keyword triangularSolves isai: row i of the approximate inverse of one triangle of the factor on the pattern J of row i
// of W (ascending, at most FACTOR_ISAI_MAX_ROW entries), by substitution over T(J, J); lanes own rows, the entries of T
// are searched in its rows.  Lower (W_L L = I on the pattern): from the diagonal, J's last entry, down; upper (ILU's U,
// W_U U = I on the pattern): from the diagonal, J's first entry, up.
constexpr int FACTOR_ISAI_MAX_ROW = 32;
void launch_factor_isai_generate(hipStream_t st, int32_t n, const DevTri &T, const int32_t *w_row_ptrs,
                                 const int32_t *w_cols, double *w_vals);
// inv_d[i] = 1 / f[diag[i]]
void launch_factor_inv_diag(hipStream_t st, int32_t n, const int32_t *diag, const double *f, double *inv_d);
// gated permutations (as launch_permute_gather / _scatter)
void launch_factor_gather_perm(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out,
                               const DevScalars *gate);
void launch_factor_scatter_perm(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out,
                                const DevScalars *gate);

// Multigrid (kernels_mg.hip; Preconditioner.H:259-341): an aggregation hierarchy generated on the device and the kernels
// of its V-cycle.  The contract is spelled out in DESIGN.md section 7b.
template <class T>
struct MgCsrOf {  // one matrix of the hierarchy: columns ascending per row
    int32_t n = 0, nnz = 0;
    const int32_t *row_ptrs = nullptr, *cols = nullptr;
    const T *vals = nullptr;
};
using MgCsr = MgCsrOf<double>;  // (MgCsrOf<float>, keyword cyclePrecision single: binary32 values on the same index arrays)
constexpr double MG_OMEGA = 0.9;  // the smoother's relaxation factor
constexpr int MG_ROUNDS = 15;     // matching rounds per coarsening
constexpr int MG_MAX_PASSES = 4;  // keyword aggregatePasses: pairwise coarsenings per kept level
struct MgScalars {                // the coarsest level's CG
    double rho, prev_rho, beta;
};
// the tail of the hierarchy as ONE single-workgroup kernel: levels first .. last of the V-cycle (the last one is the
// coarsest), walked down, solved and walked up with barriers between the phases.  b: right-hand side of the first of
// them, x: its answer; the levels' own vectors hold everything in between.  coarse_visits (keyword coarseVisits, 1 .. 3):
// every level below the first, the coarsest excepted, is visited that often per visit of its parent -- the first visit from
// nothing, the others continued from the answer before with the same right-hand side.  The first level has one visit per
// launch; continued != 0: that visit starts from what x holds (the launcher's own revisit of it) instead of from nothing.
// sweeps (keyword smootherSweeps, 1 .. 4): sweeps before and after the coarse correction on every level; scale (keyword
// correctionScale): the factor on every prolongated correction, held as a double and rounded to T in the kernel.
template <class T>
struct MgTailLevelOf {
    int32_t n = 0, n_coarse = 0;
    const int32_t *row_ptrs = nullptr, *cols = nullptr, *agg = nullptr, *agg_ptr = nullptr, *agg_rows = nullptr;
    const T *vals = nullptr, *inv_d = nullptr;
    T *b = nullptr, *xa = nullptr, *xb = nullptr, *t = nullptr, *r = nullptr, *p = nullptr;
    double *part = nullptr;  // (the partials of the coarsest CG's sums are doubles in either precision)
};
constexpr int MG_TAIL_MAX_LEVELS = 16;
constexpr int MG_TAIL_DEFAULT_ROWS = 512;  // property mgTailRows
constexpr int MG_TAIL_MAX_ROWS = 1024 * 512;  // (the finaliser's tree inside the workgroup: one partial per virtual thread)
constexpr int MG_MAX_COARSE_VISITS = 3;     // keyword coarseVisits (k_mg_tail counts a level's visits in two bits)
constexpr int MG_MAX_SWEEPS = 4;            // keyword smootherSweeps: sweeps before and after the coarse correction
constexpr int MG_MAX_VISITS_PER_APPLY = 4096;  // level visits of one apply, summed over the levels: beyond it the solve is refused
template <class T>
struct MgTailOf {
    int32_t count = 0, cg_iters = 0, coarse_visits = 1, continued = 0, sweeps = 2;
    double scale = 1.0;
    MgTailLevelOf<T> lev[MG_TAIL_MAX_LEVELS];
};
template <class T>
void launch_mg_tail(hipStream_t st, const MgTailOf<T> &Tl, const T *b, T *x, const DevScalars *gate);
// generation: diag[i] = A(i, i), inv_d[i] = 1 / A(i, i) (inv_d nullptr: not wanted)
void launch_mg_diag(hipStream_t st, const MgCsr &A, double *diag, double *inv_d);
// s[i] = strongest unaggregated (want 0) / aggregated (want 1) neighbour of the unaggregated row i (-1 none, -2 row aggregated);
// hashed: equal strengths go to the larger edge hash before the larger column (aggregation hashed)
void launch_mg_strongest(hipStream_t st, const MgCsr &A, const double *diag, const int32_t *agg, int want, bool hashed,
                         int32_t *s);
// comp[i] = cidx[comp[i]]: the aggregate map of a kept level composed from its passes
void launch_mg_compose(hipStream_t st, int32_t n, const int32_t *cidx, int32_t *comp);
// mutual pairs become aggregates; *left += rows still unaggregated
void launch_mg_match(hipStream_t st, int32_t n, const int32_t *s, int32_t *agg, int32_t *left);
void launch_mg_join(hipStream_t st, int32_t n, const int32_t *s, int32_t *agg);
void launch_mg_root_flag(hipStream_t st, int32_t n, const int32_t *agg, int32_t *flag);
void launch_mg_coarse_index(hipStream_t st, int32_t n, const int32_t *agg, const int32_t *incl, int32_t *cidx, int32_t *rows);
void launch_mg_member_ptr(hipStream_t st, int32_t n, int32_t nc, const int32_t *sorted, int32_t *agg_ptr);
void launch_mg_keys(hipStream_t st, const MgCsr &A, const int32_t *cidx, unsigned long long *keys);
void launch_mg_head_flag(hipStream_t st, int32_t m, const unsigned long long *keys, int32_t *flag);
void launch_mg_compact(hipStream_t st, int32_t m, int32_t nc, const unsigned long long *keys, const double *vals,
                       const int32_t *pos, int32_t *row_ptrs, int32_t *cols, double *out);
// keyword aggregateCaching ("kept aggregates").  A full generation keeps of every pass src -- the
// position in the pass's source matrix of the entry sorted to p, from sorting (key, index) pairs (mg_sort_entry_index of
// launch_mg_iota's identity) -- and ptr, the start of every coarse entry's run (launch_mg_run_ptr from the head flags and
// their scan).  launch_mg_regalerkin: vals_out[o] = the sum of vals_in[src[q]], q in [ptr[o], ptr[o + 1]), left to right
// from the first term -- k_mg_compact's sums without its sort; stream: src and ptr are loaded past the caches.
void launch_mg_iota(hipStream_t st, int32_t m, int32_t *idx);
void launch_mg_run_ptr(hipStream_t st, int32_t m, const int32_t *flag, const int32_t *pos, int32_t *ptr);
void launch_mg_regalerkin(hipStream_t st, int32_t mc, const int32_t *ptr, const int32_t *src, const double *vals_in,
                          double *vals_out, bool stream);
// scan and stable radix sorts (hipcub); mg_temp_bytes: scratch that serves all of them on a level of n rows, nnz entries
size_t mg_temp_bytes(int32_t n, int32_t nnz);
hipError_t mg_inclusive_sum(hipStream_t st, void *temp, size_t temp_bytes, const int32_t *in, int32_t *out, int32_t n);
hipError_t mg_sort_rows(hipStream_t st, void *temp, size_t temp_bytes, const int32_t *keys, int32_t *keys_out,
                        const int32_t *rows, int32_t *rows_out, int32_t n);
hipError_t mg_sort_entries(hipStream_t st, void *temp, size_t temp_bytes, const unsigned long long *keys,
                           unsigned long long *keys_out, const double *vals, double *vals_out, int32_t m);
hipError_t mg_sort_entry_index(hipStream_t st, void *temp, size_t temp_bytes, const unsigned long long *keys,
                               unsigned long long *keys_out, const int32_t *idx, int32_t *idx_out, int32_t m);
// apply.  The launchers of the cycle's kernels are templates over the operand type T, instantiated for double and for float
// (keyword cyclePrecision single, DESIGN.md section 7b, "the cycle in single precision": the same kernels on binary32
// operands with binary32 operations; the scalars of the coarsest CG stay doubles, formed from wide sums -- products of the
// float64 casts in the loop's tree -- and rounded once where a vector kernel takes them).  What only one precision has a
// kernel for is refused by an assert in the launcher.
// x = omega (b inv_d) | x_out = x + omega ((b - ax) inv_d) | x_out = x + scale xc[agg]
template <class T>
void launch_mg_jacobi0(hipStream_t st, int32_t n, const T *b, const T *inv_d, T *x, const DevScalars *gate);
void launch_mg_sweep_epi(hipStream_t st, int32_t n, const double *b, const double *ax, const double *inv_d, const double *x,
                         double *x_out, const DevScalars *gate);
template <class T>
void launch_mg_prolong(hipStream_t st, int32_t n, const T *x, const T *xc, const int32_t *agg, T scale, T *x_out,
                       const DevScalars *gate);
// one sweep on a CSR level (x_out != x); xc != nullptr: on t = x + scale xc[agg], the prolongation folded in;
// x_out64 != nullptr (float only): the result is written there as doubles (level 0's last post-sweep) instead of x_out
template <class T>
void launch_mg_csr_sweep(hipStream_t st, const MgCsrOf<T> &A, const T *inv_d, const T *b, const T *x, const T *xc,
                         const int32_t *agg, T scale, T *x_out, double *x_out64, const DevScalars *gate);
template <class T>
void launch_mg_csr_spmv(hipStream_t st, const MgCsrOf<T> &A, const T *x, T *y, const DevScalars *gate);
// bc[I] = sum of r_i = b_i - (A x)_i over the members of I, ascending.  from: MG_FROM_A the kernel forms the products
// itself (src unused), MG_FROM_AX src holds A x (double only), MG_FROM_RES src holds the residuals r (float only)
enum MgRestrictFrom { MG_FROM_A = 0, MG_FROM_AX = 1, MG_FROM_RES = 2 };
template <class T>
void launch_mg_restrict(hipStream_t st, int32_t nc, const int32_t *agg_ptr, const int32_t *agg_rows, const MgCsrOf<T> &A,
                        const T *b, const T *x, MgRestrictFrom from, const T *src, T *bc, const DevScalars *gate);
// r = b, x = p = 0; b64 != nullptr (float only): r = fl32(b64) (a hierarchy of one level: the CG runs on the fp64
// residual's rounding)
template <class T>
void launch_mg_cg_init(hipStream_t st, int32_t n, const T *b, const double *b64, T *r, T *x, T *p, const DevScalars *gate);
// what 0: prev_rho <- rho (1 when first), rho <- sum(part); 1: beta <- sum(part) -- in the finaliser's tree
void launch_mg_cg_fin(hipStream_t st, const double *part, int32_t n_part, int what, int first, MgScalars *s,
                      const DevScalars *gate);
template <class T>
void launch_mg_cg_step1(hipStream_t st, int32_t n, T *p, const T *r, const MgScalars *s, const DevScalars *gate);
template <class T>
void launch_mg_cg_step2(hipStream_t st, int32_t n, T *x, T *r, const T *p, const T *q, const MgScalars *s,
                        const DevScalars *gate);
// --- what only the cycle in single precision launches ---
constexpr int32_t MG_NONE_BAD = 0x7f7f7f7f;  // an overflow word nothing has lowered (set by a byte fill)
// the float operands of one level: vals32 = fl32(A.vals) (nullptr: the level keeps no matrix of its own), inv_d32 =
// fl32(inv_d); *bad = the smallest row with a value that is finite in fp64 and not in binary32
void launch_mg_twin(hipStream_t st, const MgCsr &A, const double *inv_d, float *vals32, float *inv_d32, int32_t *bad);
// level 0's first pre-sweep from the fp64 residual: b = fl32(r), x = omega32 (b inv_d)
void launch_mg_jacobi0_in(hipStream_t st, int32_t n, const double *r, const float *inv_d, float *b, float *x,
                          const DevScalars *gate);
void launch_mg_wide_dot(hipStream_t st, int32_t n, const float *a, const float *b, double *part, const DevScalars *gate);
void launch_mg_widen(hipStream_t st, int32_t n, const float *x, double *out, const DevScalars *gate);

// renumbering (keyword `renumber`): host vectors arrive in the caller's cell order
//   scatter: out[new_id[i]] = in[i]   (b, x on upload)      gather: out[i] = in[new_id[i]]   (x on copy-back)
void launch_permute_scatter(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out);
void launch_permute_gather(hipStream_t st, int32_t n, const int32_t *new_id, const double *in, double *out);

// b *= scaling (lduLduBase.H:244-252)
void launch_scale(hipStream_t st, int32_t n, double *v, double factor);
// v[i] = s->xbar
void launch_fill_xbar(hipStream_t st, int32_t n, double *v, const DevScalars *s);

// --- partial sums, one per chunk ---
void launch_partials_sum(hipStream_t st, int32_t n, const double *a, double *part);
void launch_partials_dot(hipStream_t st, int32_t n, const double *a, const double *b, double *part,
                         const DevScalars *gate);
// same for the listed chunks only (multi-rank: the chunks that hold boundary rows)
void launch_partials_dot_chunks(hipStream_t st, int32_t n, const double *a, const double *b,
                                double *part, const DevScalars *gate, const int32_t *chunk_list,
                                int32_t count);
void launch_partials_norm1(hipStream_t st, int32_t n, const double *a, double *part);
// part[c] = sum over chunk of |(b - w) - r| + |b - w|   (StoppingCriterion.C:53-61)
void launch_partials_normfactor(hipStream_t st, int32_t n, const double *b, const double *w,
                                const double *r, double *part);

// --- CG steps ([UPSTREAM] cg::initialize / step_1 / step_2) ---
// partials of rho = sum r_i z_i (z = r * inv_diag, or r when inv_diag == nullptr) and sum |r_i|
void launch_cg_rho_norm(hipStream_t st, int32_t n, const double *r, const double *inv_diag,
                        double *part_rho, double *part_norm, const DevScalars *gate);
// p = z + (rho / prev_rho) p
void launch_cg_step1(hipStream_t st, int32_t n, double *p, const double *r, const double *inv_diag,
                     const DevScalars *s);
// x += (rho/beta) p ; r -= (rho/beta) q ; then the partials of the next rho and sum |r|
void launch_cg_step2(hipStream_t st, int32_t n, double *x, double *r, const double *p,
                     const double *q, const double *inv_diag, double *part_rho, double *part_norm,
                     const DevScalars *s);

// The same steps with the x update deferred by one turn (p is then read once per turn):
//   step_2r: r -= (rho/beta) q + partials;  step_1x(turn): x += (prev_rho/beta) p_old, then step_1.
// step_1x applies the pending update of turn-1 also when the solve has just stopped.
struct HaloPutFused;  // (below, after PeerHalo)
void launch_cg_step1x(hipStream_t st, int32_t n, double *p, double *x, const double *r,
                      const double *inv_diag, const DevScalars *s, const HaloPutFused *put = nullptr);
// put (chunk_sptr != nullptr): z of the send rows goes to the neighbours (multi-rank merged turn)
void launch_cg_step2r(hipStream_t st, int32_t n, double *r, const double *q, const double *inv_diag,
                      double *part_rho, double *part_norm, const DevScalars *s, double *z_out = nullptr,
                      const HaloPutFused *put = nullptr);

// Small systems: the same pair with the finalisers folded in (kernels_krylov.hip).  Every workgroup reduces the
// per-chunk partials itself in the finaliser's order; the scalars are read from `sin` and written to `sout`.
//   step_1x_fin: check on (part_rho, part_norm) of the previous step_2r (first: of the initial residual), the
//                pending x update (not when `first`), then step_1
//   step_2r_fin: beta from part_beta, then step_2r
// lead.box != nullptr (any number of chunks): workgroup 0 alone reduces and publishes, the others poll (LeadBox)
void launch_cg_step1x_fin(hipStream_t st, int32_t n, double *p, double *x, const double *r, const double *inv_diag,
                          const DevScalars *sin, DevScalars *sout, const double *part_rho,
                          const double *part_norm, double *history, int first, const LeadBox &lead = LeadBox{},
                          double *p_out = nullptr, const PRing &ring = PRing{});  // (ring.k > 0: x touched every k-th turn, see the kernel)
void launch_cg_step2r_fin(hipStream_t st, int32_t n, double *r, const double *q, const double *inv_diag,
                          double *part_rho, double *part_norm, const DevScalars *sin, DevScalars *sout,
                          const double *part_beta, double *z_out = nullptr,  // z_out: z = r / d kept for k_cg_turn_sym
                          const LeadBox &lead = LeadBox{});
// The held-z turn (kernels_krylov.hip, k_cg_step2r1x): step_2r_fin of a turn and step_1x_fin of the next in one resident
// kernel that keeps z = r / d on chip.  `s` is read and rewritten in place; launch_seq advances by two.  Its phases behind
// the sum of beta are one body with the held-q turn's (resident_cg_turn.hpp); the check in it, as in every kernel that
// checks, is criterion_verdict (device_common.hpp).
struct HeldZ {
    unsigned long long *tagged = nullptr;  // 4 words per chunk, fine-grained: the chunk's two partials as tagged half-words
    int32_t grid = 0;                      // workgroups, all resident at once; each owns chunks w, w + grid, ...
    int32_t early_slots = 0;               // a head that updates x does so for its first early_slots slots while the sums are
                                           // awaited, for the others in the loop that forms p_new (0: for all of them there)
};
// the geometry both resident turn kernels share: B workgroups per CU, R chunks per workgroup held in registers, L in LDS
constexpr int HZ_B = 4, HZ_R = 11, HZ_L = 9;
int held_z_grid(int *chunks_per_workgroup);  // the largest resident grid of the kernels on this device (0: none)
// every workgroup of `grid` waits, bounded, for all the others: *out = 1 afterwards when they were not all on the chip at once
int launch_resident_census(hipStream_t st, int grid, unsigned *arrived, int *out, long long timeout_ticks);
void launch_cg_step2r1x(hipStream_t st, int32_t n, double *r, const double *q, const double *inv_diag, double *p,
                        double *p_out, double *x, DevScalars *s, const double *part_beta, double *history,
                        const LeadBox &lead, const PRing &ring, const HeldZ &hz);
// The held-q turn (kernels_spmv_sym.hip, k_cg_turn_held_q): the half-storage SpMV in front of that kernel's body, one
// launch per turn -- q = A p stays on chip across the sum beta = p.q as z does across the later two.  The workgroups own
// POSITIONS of the layout's launch order (slot i of workgroup w: position w + i grid), so the tagged box has 6 words per
// chunk.
struct HeldQ {
    int32_t on = 0;     // 1: the turns without an event pair run the one-launch kernel
    int32_t n_pos = 0;  // positions of the launch order (DevSym::n_blocks, or xcd_grid(chunks) without a band order)
    // Phase S draws (property heldQStaticSlots): slot i < static_slots of workgroup w holds position w + i grid, the
    // positions from static_slots * grid on form eight queues (position p: queue p % 8) that the first `drawers`
    // workgroups draw from, workgroup w from queue w % 8.  static_slots == HQ_STATIC: every slot static, no counter
    // touched.  heads: 2 sets of 8 counters, one 128-byte line each; launch j draws from set `parity` and zeroes the
    // other -- parity counts the held-q LAUNCHES of the solve (turn_cg_held_q).
    int32_t static_slots = 0;
    int32_t drawers = 0;
    unsigned *heads = nullptr;
    int32_t parity = 0;
};
// The held-q kernel's own register slots: HQ_R + HZ_L = 22 slots per workgroup at the occupancy and LDS of 11 + 9.  The
// two slots more are headroom for the draw to balance with, not capacity: the gates stay at grid * HQ_STATIC positions.
constexpr int HQ_R = 13, HQ_STATIC = HZ_R + HZ_L;
// heldQStaticSlots where the property is not set.  Measured at 216^3 (profiles/r14_held_q_draw.txt): 4 .. 14 run level,
// 2.4 % above the static map; 16, 0 and 18 gain less or nothing
constexpr int HQ_STATIC_DEFAULT = 12;
constexpr int HQ_HEAD_STRIDE = 32, HQ_HEAD_WORDS = 2 * N_XCD * HQ_HEAD_STRIDE;  // (unsigned words: 128 bytes per counter)
int held_q_positions(const DevSym &A);
// occupancy (workgroups per CU) and static LDS bytes of the held-q instantiations: the minimum / the maximum over them
int held_q_occupancy(int *per_cu, size_t *lds_bytes);
void launch_cg_turn_held_q(hipStream_t st, const DevSym &A, double *r, const double *inv_diag, double *p, double *p_out,
                           double *x, DevScalars *s, double *history, const LeadBox &lead, const PRing &ring,
                           const HeldZ &hz, const HeldQ &hq);
constexpr int FUSED_FIN_MAX_CHUNKS = 1024;  // up to 524,288 rows: one partial per virtual finaliser thread
// step_1x_fin and the SpMV on half storage in one launch (p_new = z + (rho/rho') p recomputed at the gathered
// columns; it goes to p_out != p_in for the own rows): a turn is this + step_2r_fin.  z: what step_2r_fin's z_out
// (or, before the first turn, launch_mul) has left; r itself without a preconditioner
void launch_cg_turn_sym(hipStream_t st, const DevSym &A, const double *p_in, double *p_out, double *x, const double *z,
                        double *q, double *part_beta, const DevScalars *sin, DevScalars *sout,
                        const double *part_rho, const double *part_norm, double *history, int first,
                        const LeadBox &lead = LeadBox{});
// ... and between the single-workgroup finalisers of larger systems (scalars as k_cg_step1x reads them):
// turn = this | FIN_BETA | step_2r (z_out) | FIN_CG_CHECK
// Several ranks (hf.chunk_bptr != nullptr; peer-put transport): the neighbours have put the z of the halo columns
// (step_2r's `put`, launch_pack_put_signal before the first turn); p_halo_in = this rank's copy of the OLD p at its
// halo columns (zero before the first turn), p_halo_out receives the new one:
// turn = this (waits for z, nothing to put) | FIN_BETA | step_2r (z_out, puts z) | FIN_CG_CHECK
void launch_cg_turn_sym_big(hipStream_t st, const DevSym &A, const double *p_in, double *p_out, double *x,
                            const double *z, double *q, double *part_beta, const DevScalars *s,
                            const HaloFused &hf = HaloFused{}, const double *p_halo_in = nullptr,
                            double *p_halo_out = nullptr);

// --- BiCGStab steps ([UPSTREAM] bicgstab::step_1/2/3, finalize) ---
// a Gram-Schmidt link with the finaliser of the PREVIOUS link folded in (<= FUSED_FIN_MAX_CHUNKS chunks, one rank):
// vprev != nullptr: H = sum(part_in) -> *h_out, w -= H vprev; then the partials of w . vdot (w . w when vdot is nullptr)
void launch_gmres_mgs_fold(hipStream_t st, int32_t n, double *w, const double *vprev, double *h_out, const double *vdot,
                           const double *part_in, double *part_out, const DevScalars *gate, const LeadBox &lead = LeadBox{},
                           uint32_t tag = 0);  // (lead.box: leader finalisation, tag = a number no earlier launch of the solve used)
// GKOBiCGStab with the finalisers folded into the step kernels (<= FUSED_FIN_MAX_CHUNKS chunks, one rank; kernels_krylov.hip):
// scalars go sin -> sout; a kernel never writes a partial array it reads
void launch_bicg_fold1(hipStream_t st, int32_t n, double *p, const double *r, const double *v, const double *inv_diag,
                       double *y, const DevScalars *sin, DevScalars *sout, const double *part_rho,
                       const double *part_norm, double *history, const LeadBox &lead = LeadBox{});
void launch_bicg_fold2(hipStream_t st, int32_t n, const double *r, const double *v, double *sv, const double *inv_diag,
                       double *z, double *part_norm_out, const DevScalars *sin, DevScalars *sout,
                       const double *part_beta, const LeadBox &lead = LeadBox{});
void launch_bicg_fold3(hipStream_t st, int32_t n, double *x, double *r, const double *sv, const double *t,
                       const double *y, const double *z, const double *rr, double *part_rho_out, double *part_norm_out,
                       const DevScalars *sin, DevScalars *sout, const double *part_gamma, const double *part_tt,
                       const double *part_snorm, double *history, int turn, const LeadBox &lead = LeadBox{});
void launch_bicg_step1(hipStream_t st, int32_t n, double *p, const double *r, const double *v,
                       const double *inv_diag, double *y, const DevScalars *s);
void launch_bicg_step2(hipStream_t st, int32_t n, const double *r, const double *v, double *sv,
                       const double *inv_diag, double *z, double *part_norm, const DevScalars *s);
void launch_bicg_step3(hipStream_t st, int32_t n, double *x, double *r, const double *sv,
                       const double *t, const double *y, const double *z, const double *rr,
                       double *part_rho, double *part_norm, const DevScalars *s, int turn);
// (step_3 of the turn whose mid-step check stopped the solve applies bicgstab::finalize,
//  x += alpha y, instead of its own work)

// --- GMRES vector kernels ([UPSTREAM] gmres::restart / finish_arnoldi / solve_krylov) ---
// out = in / *denom
// out = in / *denom and w = out * inv_diag in one pass (scalar Jacobi: the scaling of a new basis vector waits for the
// turn that applies the preconditioner to it)
void launch_gmres_scale_mul(hipStream_t st, int32_t n, double *out, const double *in, const double *denom,
                            const double *inv_diag, double *w, const DevScalars *gate);
void launch_gmres_scale(hipStream_t st, int32_t n, double *out, const double *in,
                        const double *denom, const DevScalars *gate);
// modified Gram-Schmidt link: if (vprev) w -= (*hprev) * vprev ; partial of w . vdot (vdot == nullptr: w . w)
void launch_gmres_mgs(hipStream_t st, int32_t n, double *w, const double *vprev,
                      const double *hprev, const double *vdot, double *part,
                      const DevScalars *gate);
// classical Gram-Schmidt in block form (kernels_gmres.hip; orthoMethod cgs | cgs2).  V: the basis,
// vector j at V + j * ld; k = it + 1 vectors take part; a partial array holds row j at part + j * n_chunks(n).
// multidot: the partials of w . V_j, j < k.  fin_h (one workgroup per j, k_finalize's tree): h[j] = sum of row j, and
// h_col[j] = h[j] (add: h_col[j] + h[j]).  block_update: w -= sum_j h[j] V_j, j ascending; then the partials of w . w into
// part_norm, or (part_dots != nullptr) those of w . V_j on the new w into part_dots.
// (a `const float *V`: the basis stored in fp32, property basisPrecision single -- DESIGN.md section 7e; each entry is
//  widened exactly where it is loaded and the arithmetic is the double one)
void launch_gmres_multidot(hipStream_t st, int32_t n, const double *w, const double *V, int64_t ld, int32_t k, double *part,
                           const DevScalars *gate);
void launch_gmres_multidot(hipStream_t st, int32_t n, const double *w, const float *V, int64_t ld, int32_t k, double *part,
                           const DevScalars *gate);
void launch_gmres_fin_h(hipStream_t st, int32_t n, const DevScalars *gate, const double *part, int32_t k, double *h,
                        double *h_col, bool add);
void launch_gmres_block_update(hipStream_t st, int32_t n, double *w, const double *V, int64_t ld, int32_t k, const double *h,
                               double *part_norm, double *part_dots, const DevScalars *gate);
void launch_gmres_block_update(hipStream_t st, int32_t n, double *w, const float *V, int64_t ld, int32_t k, const double *h,
                               double *part_norm, double *part_dots, const DevScalars *gate);
// t_i = sum_{j < it} V_j[i] * y[j] ; with `before` != nullptr the sum is stored there, otherwise
// x_i += t_i * inv_diag_i (inv_diag == nullptr: x_i += t_i)
void launch_gmres_update_x(hipStream_t st, int32_t n, const double *V, int64_t ld, const double *y,
                           int32_t it, const double *inv_diag, double *x, double *before,
                           const DevScalars *gate);
void launch_gmres_update_x(hipStream_t st, int32_t n, const float *V, int64_t ld, const double *y, int32_t it,
                           const double *inv_diag, double *x, double *before, const DevScalars *gate);
// basisPrecision single, the head of a turn: v_out = fl32(in / *denom) as floats and w = wide(v_out) (inv_diag != nullptr:
// times inv_diag), in place of launch_gmres_scale / launch_gmres_scale_mul
void launch_gmres_head_f32(hipStream_t st, int32_t n, float *v_out, const double *in, const double *denom,
                           const double *inv_diag, double *w, const DevScalars *gate);
// The initial guess from the stored steps of the last solves (kernels_proj.hip; keyword guessProjection, DESIGN.md section
// 7f).  W: w_j = A d_j at W + j * ld, j < k <= PROJ_MAX.  gram: one pass over r0 and W, the partials of the proj_n_sums(k)
// sums S0 = sum |r0| | g_j = w_j . r0 | G_ij = w_i . w_j (i >= j, row by row), row s of the partial array at part + s *
// n_chunks(n); launch_gmres_fin_h reduces them.  solve (one thread): Cholesky with dropping of G, h[j] = -alpha_j for
// launch_gmres_block_update, rec = {S0, columns kept, k}.  delta: d = x - x0, one rounded difference per row.
constexpr int PROJ_MAX = 8;
int proj_n_sums(int k);
void launch_proj_gram(hipStream_t st, int32_t n, const double *r0, const double *W, int64_t ld, int32_t k, double *part,
                      const DevScalars *gate);
void launch_proj_solve(hipStream_t st, int32_t k, const double *sums, double *h, double *rec, const DevScalars *gate);
void launch_proj_delta(hipStream_t st, int32_t n, const double *x, const double *x0, double *d, const DevScalars *gate);
// keyword guessProjectionProducts onePass (kernels_spmv_sym.hip): r0 = b - A x0 and W + j * ld = A in[j], j < k, in one pass
// over the half storage; the bits of launch_spmv_sym's k + 1 products
struct ProjProducts {
    const double *in[PROJ_MAX];
    double *W;
    long ld;
    int k;
};
void launch_proj_products_sym(hipStream_t st, const DevSym &A, const double *x0, const double *b, double *r0,
                              const ProjProducts &v);
// keyword guessProjectionCredit: s->init_res = rec[0] (S0) when a column was kept and S0 is finite and > 0, else 0 -- after
// launch_reset_scalars and before the solve's first check (criterion_verdict, device_common.hpp)
void launch_proj_credit(hipStream_t st, const double *rec, DevScalars *s);
// Preconditioner Chebyshev (kernels_cheb.hip): z = p(D^-1 A) D^-1 r with the Chebyshev polynomial of
// [lambda_max / ratio, lambda_max].  The table lives in the preconditioner object and the apply's kernels read it through
// the pointer, never from launch arguments: a regeneration changes the numbers under launches that stay what they were.
constexpr int CHEB_MAX_DEGREE = 16;
struct ChebTable {
    double lambda_max, lambda_min;  // lambda_max: first the running maximum of k_cheb_bound (as its bit pattern)
    double c0;                      // 1 / theta
    double a[CHEB_MAX_DEGREE], b[CHEB_MAX_DEGREE];  // step k = 1 .. degree: a[k - 1] = rho_k rho_(k-1), b[k - 1] = 2 rho_k / delta
    int32_t breakdown, pad_;        // 1: lambda_max is not finite or not positive
};
// tab->lambda_max = max over the rows of (sum_j |a_ij|, stored order, from 0) / |a_ii| (not finite: +inf); the caller
// has zeroed it.  diag_pos: position of each row's diagonal entry (-1: none)
void launch_cheb_bound(hipStream_t st, const DevCsr &A, const int32_t *diag_pos, ChebTable *tab);
// one thread: the table for `degree` steps from tab->lambda_max (forced > 0: from that instead) and the ratio
void launch_cheb_coeffs(hipStream_t st, int32_t n_rows, int32_t degree, double ratio, double forced, ChebTable *tab);
// z1 = (r w) c0
void launch_cheb_first(hipStream_t st, int32_t n, const double *r, const double *w, const ChebTable *tab, double *z1,
                       const DevScalars *gate);
// One step of the recurrence, z_next = (z + a_k (z - z_prev)) + b_k (w t) with t = r - A z: z_io holds z_prev (k == 1:
// nothing, z_prev = 0) and receives z_next.  dot_part != nullptr: also the per-chunk partials of r . z_next.
// launch_cheb_step: t comes from a product kernel; launch_cheb_step_sym: formed here on the half storage (the same bits)
void launch_cheb_step(hipStream_t st, int32_t n, int32_t k, const double *t, const double *w, const ChebTable *tab,
                      const double *z, double *z_io, const double *r, double *dot_part, const DevScalars *gate);
void launch_cheb_step_sym(hipStream_t st, const DevSym &A, int32_t k, const double *r, const double *w, const ChebTable *tab,
                          const double *z, double *z_io, double *dot_part, const DevScalars *gate);
// The Krylov basis a GKOGMRES solve works on: one of the two is set (launch_key.hpp hashes it)
struct GmresBasis {
    const double *V = nullptr;  // basisPrecision double
    const float *Vf = nullptr;  // basisPrecision single
    int64_t ld = 0;             // leading dimension, in elements of the stored type
    int32_t single = 0, pad_ = 0;
};
// out = in * inv_diag (scalar Jacobi apply), x += a
void launch_mul(hipStream_t st, int32_t n, double *out, const double *in, const double *inv_diag,
                const DevScalars *gate);
void launch_add(hipStream_t st, int32_t n, double *x, const double *a, const DevScalars *gate);

// --- single-workgroup finalisers: reduce per-chunk partials, then scalar logic -------------
// phases: what the scalar logic does with the reduced sums.
enum FinPhase {
    FIN_MEAN = 0,        // xbar = sum/n * n/global_n (all-reduced)        StoppingCriterion.C:17-19
    FIN_NORMFACTOR = 1,  // norm_factor = sum + SMALL                      StoppingCriterion.C:62-68
    FIN_CG_CHECK = 2,    // rho <- sum0, criterion check on sum1           StoppingCriterion.C:71-151
    FIN_BETA = 3,        // beta <- sum0
    FIN_RAW = 4,         // sums[] only (test / reduce entry point)
    FIN_BICG_ALPHA = 5,  // beta <- sum0 ; alpha = rho / beta
    FIN_BICG_CHECK2 = 6, // mid-turn criterion check on sum0 = sum|s|
    FIN_BICG_OMEGA = 7,  // gamma <- sum0 ; beta <- sum1 ; omega = gamma / beta
    // (the criterion check of a GKOGMRES turn -- on stale_norm, the sum|r| of the last restart -- has no launch of its own:
    //  FinArgs::check_after runs it at the end of the finaliser before it, restart or column)
    FIN_GMRES_RESTART = 8,  // rn = sqrt(sum0) -> rnc[0], beta ; stale_norm = sum1   (gmres::restart)
    FIN_GMRES_H = 9,        // H(k, it) = sum0                                        (finish_arnoldi)
    FIN_GMRES_COL = 10,     // H(it+1, it) = sqrt(sum0) -> beta ; Givens ; rnc        (givens_rotation)
    FIN_GMRES_SOLVE = 12,   // y = R^-1 rnc for `turn` columns                        (solve_krylov)
    // single rank: FIN_BICG_CHECK2 and FIN_BICG_OMEGA in one launch, after the second SpMV (which then runs even when
    // the mid-turn check stops the solve: its result is not used); sums: s.t, t.t and, from part_extra, sum|s|
    FIN_BICG_CHECK2_OMEGA = 13
};
// GMRES small dense state in one device array of doubles:
//   H[(m+1) x m] column-major | givens_sin[m] | givens_cos[m] | rnc[m+1] | y[m]
inline size_t gmres_state_len(int m) { return (size_t)(m + 1) * m + 2 * (size_t)m + (m + 1) + m; }
// Peer-write all-reduce over xGMI (SURVEY.md §8e "peer-write mesh all-reduce"): every rank owns a
// small mailbox in fine-grained device memory that all ranks have mapped (hipIpc).  All-reduce
// number `seq`: a rank stores its values into column `rank` of slot seq % PEER_SLOTS of EVERY
// mailbox, as 64-bit words (32 data bits | seq << 32) so that data and flag arrive in one atomic
// store, then reads its own mailbox until every column carries `seq`, and adds the columns in rank
// order -- every rank gets the same bits.  It runs INSIDE the finaliser kernel: no extra launch,
// no host, no collective library on the latency path of the two reductions per CG turn.
constexpr int PEER_MAX_RANKS = 16;
// a rank that does not show up within this time fails the solve with OGL_ERR_COMM instead of
// hanging the GPU (OGL_PEER_TIMEOUT_S overrides the 60 s)
constexpr long long PEER_DEFAULT_TIMEOUT_TICKS = 60LL * 100000000LL;
constexpr int PEER_SLOTS = 4;
constexpr int PEER_ELEMS = 4;  // two doubles as four half-words
constexpr size_t PEER_BOX_WORDS = (size_t)PEER_SLOTS * PEER_MAX_RANKS * PEER_ELEMS;
struct PeerArgs {
    int32_t world = 0;  // 0 / 1: no exchange
    int32_t rank = 0;
    uint32_t seq = 0;   // never 0 (the mailboxes start zeroed)
    long long timeout_ticks = PEER_DEFAULT_TIMEOUT_TICKS;  // of the 100 MHz wall clock
    unsigned long long *box[PEER_MAX_RANKS] = {};  // mailbox of rank q as mapped in this process
};
// vals[0..n) (n <= 2, device memory) summed over the ranks in place; *error set on timeout
void launch_peer_allreduce(hipStream_t st, const PeerArgs &pa, double *vals, int n, int32_t *error);

// Peer-put halo exchange (SURVEY.md §8e "pack x[send_idxs] then peer-to-peer put to each neighbour
// over xGMI").  A rank's IPC allocation is [mailbox | control slots | arena]; every solver with
// processor interfaces owns an arena block [flags 2 x n_neigh | recv parity 0 | recv parity 1].
// SpMV number `seq` of a solver, every step written once for 8-byte values (the double path) and 4-byte values (the inner
// product of the mixed mode, which views the same receive blocks as floats):
//   put    x[send_idxs] goes straight into the neighbours' recv segments of parity seq & 1, every workgroup fences its
//          stores at system scope and takes a ticket, and the last one stores `seq` into the neighbours' flags for this
//          rank: k_pack_put_signal -- or the kernel that produces x, for the chunks it owns (HaloPutFused below)
//   local  the local SpMV runs while the values fly
//   wait + non-local, one of
//          inside the local kernel: the workgroup of a chunk with boundary rows polls this rank's flags until all
//            carry `seq`, then continues those rows over their non-local entries (HaloFused; the default, doubles only)
//          k_halo_finish, one workgroup per such chunk: the same, then the chunk's dot partials (haloFused 0, mixed mode)
//          k_halo_wait, ONE workgroup; then k_spmv_non_local over the boundary rows and the boundary chunks' partials
//            again (peerSafeWait: ranks that share a device)
// Two parities: a neighbour can be at most one SpMV ahead.  The other transports pack into a send buffer of doubles
// (k_pack), exchange it through Comm and run k_spmv_non_local on the arrived block.
constexpr size_t PEER_CTRL_WORDS = (size_t)PEER_MAX_RANKS * 4;  // per source rank: epoch + 3 words
constexpr size_t PEER_ARENA_OFF = PEER_BOX_WORDS + PEER_CTRL_WORDS;  // 8-byte words from the base
constexpr int PEER_MAX_NEIGH = 16;
struct PeerHalo {
    HaloWait wait{nullptr, 0, 0, PEER_DEFAULT_TIMEOUT_TICKS};
    int32_t send_off[PEER_MAX_NEIGH + 1] = {};             // send buffer blocks, by neighbour
    void *remote_recv[PEER_MAX_NEIGH] = {};                // neighbour i's segment for this rank, values of one width
    unsigned long long *remote_flag[PEER_MAX_NEIGH] = {};  // neighbour i's flag for this rank
    template <class T>
    __host__ __device__ T *segment(int i) const { return static_cast<T *>(remote_recv[i]); }
};
// Whose exchange it is: the gate its kernels return on (may be nullptr) and the scalars that take the outcome of a wait
// -- the wait's length, and comm_error with the stops when a neighbour does not show up within the time-out
// (device_common.hpp: halo_gated, halo_wait_outcome).
struct MixedScalars;
struct HaloOwner {  // the double path
    const DevScalars *gate = nullptr;
    DevScalars *s = nullptr;
};
struct MixedHaloOwner {  // the inner product of the mixed mode: both stops in `m`, the stop of `s`
    const MixedScalars *gate = nullptr;
    MixedScalars *m = nullptr;
    DevScalars *s = nullptr;
};
// launch_cg_step1x's `put` (chunk_sptr != nullptr): the workgroups whose chunks hold send rows store the p they
// have just formed straight into the neighbours' receive blocks, and the last of them signals -- the pack kernel
// of the SpMV that follows is folded into the kernel that produces its input.
struct HaloPutFused {
    PeerHalo P;
    const int32_t *chunk_sptr = nullptr;  // [n_chunks + 1] ranges of send_pos per chunk
    const int32_t *send_pos = nullptr;    // positions in the send list, grouped by the chunk of their row
    const int32_t *send_idxs = nullptr;   // the send list (rows), as DevHalo
    unsigned *ticket = nullptr;
    int32_t n_put_chunks = 0;             // chunks that hold send rows
};
// The launches of the steps above (kernels_comm.hip), instantiated for <double, HaloOwner> and <float, MixedHaloOwner>.
// Every kernel returns at once past a stop of own.gate.  nl_vals: the non-local coefficients as T (DevHalo::vals or
// their fp32 twin); H.vals itself is not read.
// put + signal by the last workgroup (P made for values of sizeof(T): ogl_solver::next_exchange)
template <class T, class Owner>
void launch_pack_put_signal(hipStream_t st, const DevHalo &H, const PeerHalo &P, const T *x, const Owner &own,
                            unsigned *ticket);
// wait + y (+/-)= A_non_local recv + the dot partials of the chunks that hold boundary rows, over the finished y (one
// workgroup per such chunk; chunk_row_ptr = ranges of H.boundary_rows per listed chunk); a time-out leaves y the local product
template <class T, class Owner>
void launch_halo_finish(hipStream_t st, const DevHalo &H, const T *nl_vals, int mode, int32_t n_rows,
                        const int32_t *chunk_list, const int32_t *chunk_row_ptr, int32_t n_chunks_b, const T *recv, T *y,
                        const SpmvDotsOf<T> &dots, const PeerHalo &P, const Owner &own);
// the single waiting workgroup of a rank
template <class Owner>
void launch_halo_wait(hipStream_t st, const PeerHalo &P, const Owner &own);
// y[row] (+/-)= sum_k nl_vals[k] * (T)recv[cols[k]] over the boundary rows, continuing y's accumulator; R = T (a receive
// block of the peer mesh) or double (the block Comm::exchange filled, narrowed on read for T = float)
template <class T, class R, class Owner>
void launch_spmv_non_local(hipStream_t st, const DevHalo &H, const T *nl_vals, int mode, const R *recv, T *y,
                           const Owner &own);
// send[j] = (double)x[send_idxs[j]]: Comm::exchange carries doubles (exact both ways for T = float)
template <class T, class Owner>
void launch_pack(hipStream_t st, const DevHalo &H, const T *x, double *send, const Owner &own);
// control message to another rank: dst[1..3] = w1..w3, then dst[0] = w0 (the epoch)
void launch_peer_post(hipStream_t st, unsigned long long *dst, unsigned long long w0,
                      unsigned long long w1, unsigned long long w2, unsigned long long w3);

struct FinArgs {
    PeerArgs peer{};  // world > 1: all-reduce the sums inside the kernel (do_reduce && do_logic)
    const double *part[2] = {nullptr, nullptr};
    const double *part_extra = nullptr;  // third partial array (FIN_BICG_CHECK2_OMEGA)
    int32_t n_part = 0;     // entries per partial array
    int32_t n_sums = 1;     // 1 or 2 (3 with part_extra)
    int32_t do_reduce = 1;  // reduce partials -> s->sums
    int32_t do_logic = 1;   // scalar logic from s->sums (after the all-reduce when multi-rank)
    double n_local = 0, n_global = 0;  // FIN_MEAN
    double *history = nullptr;
    int32_t turn = 0;  // BiCGStab turn index (FIN_BICG_CHECK2); GMRES: column `it`
    double *gm = nullptr;  // GMRES dense state
    int32_t m = 0;         // GMRES krylov_dim
    int32_t k = 0;         // GMRES row of H (FIN_GMRES_H)
    int32_t check_after = 0;  // FIN_GMRES_RESTART / FIN_GMRES_COL: the criterion check of the turn that follows, in the same launch
};
void launch_finalize(hipStream_t st, int phase, DevScalars *s, const FinArgs &a);

// cg::initialize scalars: rho = 0? (unused), prev_rho = 1, iter = 0, stop = 0, norm_factor = 1
void launch_reset_scalars(hipStream_t st, DevScalars *s, const DevCriterion &crit);

// --- mixed precision for GKOCG (kernels_mixed.hip; the contract: DESIGN.md section 7c) ---
// fp32 inner CG on an fp32 copy of the matrix under an fp64 iterative refinement.  The scalars of both loops, resident on
// the device like DevScalars: every inner kernel returns at once when inner_stop or outer_stop is set, the outer kernels
// (the double path's own) gate on DevScalars::stop, which the outer check raises together with outer_stop.
enum MixedStop { MIXED_STOP_CRITERION = 0, MIXED_STOP_MAX_ITER = 1, MIXED_STOP_NO_PROGRESS = 2, MIXED_STOP_BREAKDOWN = 3,
                 MIXED_STOP_INVALID = 4 /* a value not representable in binary32: the solve fails */ };
struct MixedScalars {
    double rho, prev_rho, pi, tau, tau0;  // inner CG: wide sums (fp64)
    double theta;                         // this outer step's inner tolerance on tau / tau0
    double S, S_prev;                     // sum |r| of the fp64 residual at this / the previous outer check
    double norm_factor, init_res, res;    // the criterion's (the double path's norm factor)
    double inner_rel_tol;                 // keyword innerRelTol
    float a32, b32;                       // fl32(rho / pi), fl32(rho / rho_prev)
    int32_t use_beta;                     // 0: p = z (first turn of an inner solve, rho_prev == 0)
    int32_t inner_stop, inner_turns, inner_cap, inner_nonfinite;
    int32_t outer_stop, stop_reason, outer_steps, total_turns, n_evals;
    int32_t bad_coef, bad_invd;           // first matrix value / inverse-diagonal row that overflows binary32 (INT_MAX: none)
    int32_t inner_max_iter;               // keyword innerMaxIter
    DevCriterion crit;
    // several ranks: the rank's sums of a finaliser staged for the all-reduce of the RCCL / host-buffer rungs; the number
    // of overflow words set over all ranks (the first outer check's all-reduce carries it next to S); a neighbour or a
    // rank that did not show up within the time-out (the solve fails with OGL_ERR_COMM); where the turns waited, as
    // DevScalars counts it for the double path
    double sums[2];
    int32_t bad_global, comm_error;
    uint32_t halo_waits, reduce_waits;
    unsigned long long halo_wait_ticks, reduce_wait_ticks;
};
// out[i] = fl32(src[map[i]]) (0 where map[i] < 0; map == nullptr: src[i]); *bad = min(*bad, base + i) where a finite value
// overflows (base: the non-local coefficients report positions behind the local ones)
void launch_mixed_refresh(hipStream_t st, int64_t n, const int32_t *map, const double *src, float *out, int32_t *bad,
                          int64_t base = 0);
void launch_mixed_reset(hipStream_t st, MixedScalars *m, const DevCriterion &crit, double inner_rel_tol, int inner_max_iter);
// y = A32 x on the fp32 twin of the half storage's planes / on the fp32 value array beside the device CSR; every row from
// 0.0f in ascending column order.  part != nullptr: the per-chunk partials of sum (double)x_i (double)y_i
// Multigrid's cycle in single precision runs its fine level on the same products with an epilogue in place of the pi
// partials (MgEpi; gated by the Krylov loop's stop flag instead of the mixed mode's):
//   MX_EPI_PLAIN y = A x | _SWEEP out = x + omega32 ((b - A x) inv_d) | _RESIDUAL out = b - A x | _SWEEP64 the sweep, written
//   as doubles to out64
enum MxEpilogue { MX_EPI_PI = 0, MX_EPI_PLAIN, MX_EPI_SWEEP, MX_EPI_RESIDUAL, MX_EPI_SWEEP64 };
struct MgEpi {
    const float *b = nullptr, *inv_d = nullptr;
    float *out = nullptr;
    double *out64 = nullptr;
    const DevScalars *gate = nullptr;
};
void launch_mg_fine_sym(hipStream_t st, const DevSym &A, const float *planes, MxEpilogue epi, const float *x, const MgEpi &e);
void launch_mg_fine_csr(hipStream_t st, const DevCsr &A, const float *vals, MxEpilogue epi, const float *x, const MgEpi &e);
void launch_mixed_spmv_sym(hipStream_t st, const DevSym &A, const float *planes, const float *x, float *y, double *part,
                           const MixedScalars *gate);
void launch_mixed_spmv_csr(hipStream_t st, const DevCsr &A, const float *vals, const float *x, float *y, double *part,
                           const MixedScalars *gate);
// The four finalisers of the mode (one workgroup each): the check of an outer step on the partials of sum |r| with the
// step's inner tolerance and budget (HEAD; `s`: the double path's scalars, `history`), and the inner solve's START (rho,
// tau0) | PI (pi, a32) | RHO (rho, tau, b32, the inner stop gate).  Several ranks: the sums -- S and the overflow count |
// rho, tau0 | pi | rho, tau -- are all-reduced between the reduction and the logic, inside the launch on the peer mesh
// (peer.world > 1), else by the caller between a do_reduce and a do_logic launch (MixedScalars::sums), as FinArgs has it.
enum MixedFin { MIXED_FIN_HEAD = 0, MIXED_FIN_START = 1, MIXED_FIN_PI = 2, MIXED_FIN_RHO = 3 };
struct MixedFinArgs {
    PeerArgs peer{};
    const double *part[2] = {nullptr, nullptr};
    int32_t n_part = 0;
    int32_t do_reduce = 1, do_logic = 1;
    double *history = nullptr;
};
void launch_mixed_fin(hipStream_t st, int phase, MixedScalars *m, DevScalars *s, const MixedFinArgs &a);
// r32 = fl32(r / S), z = r32 * inv_d (inv_d == nullptr: z is r32 itself and not written), u = 0; the partials of rho, tau0
void launch_mixed_start(hipStream_t st, int32_t n, const double *r, const float *inv_d, float *r32, float *z, float *u,
                        double *part_rho, double *part_tau, MixedScalars *m);
void launch_mixed_step1(hipStream_t st, int32_t n, float *p, const float *z, const MixedScalars *m);
// u += a p, r -= a q, z = r * inv_d; the partials of rho, tau
void launch_mixed_step2(hipStream_t st, int32_t n, float *u, float *r, const float *p, const float *q, const float *inv_d,
                        float *z, double *part_rho, double *part_tau, MixedScalars *m);
// (The halo of the inner product on several ranks: the launches of the peer-put exchange above with <float, MixedHaloOwner>.)
// launch_partials_dot_chunks for the inner product's operands: the pi partials of the listed (boundary) chunks, formed
// again over the finished q in the local kernels' tree (k_mx_pi_chunks)
void launch_partials_dot_chunks(hipStream_t st, int32_t n, const float *x, const float *y, double *part,
                                const MixedScalars *gate, const int32_t *chunk_list, int32_t n_list);
void launch_mixed_add(hipStream_t st, int32_t n, double *x, const float *u, const MixedScalars *m);
// scatter: out[new_id[i]] = in[i]; gather: out[i] = in[new_id[i]]
void launch_mixed_permute(hipStream_t st, int32_t n, const int32_t *new_id, const float *in, float *out, bool gather);

}  // namespace ogl
