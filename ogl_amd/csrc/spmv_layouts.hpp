// spmv_layouts.hpp -- the device layouts of a CSR matrix that an SpMV kernel may run on instead of the CSR arrays, one
// owner type per layout.  An owner holds its buffers and what its kernels need besides them; it is built once per
// sparsity pattern, gathers its values from the CSR values (`refresh`) and hands out its kernel's view.  `epoch` names
// the coefficient upload its values were gathered from (ogl_solver::vals_epoch, refresh_values).  Which layout the
// in-loop SpMV of a solver runs on is ogl_solver::spmv_layout, set in one place: select_spmv_layout (solver.cpp).
#pragma once
#include <map>
#include <string>

#include "devmem.hpp"
#include "host_matrix.hpp"
#include "kernels.hpp"
#include "setup_kernels.hpp"

namespace ogl {

using Props = std::map<std::string, double>;  // a solver's properties (what the builders report)

// property spmvLayout: Csr 0, Ell 1, Sell / Sym / Symx 2 (symmetricHalf / symmetricHalfPerChunk tell them apart), Csr21 3
enum class SpmvLayout { Csr, Csr21, Ell, Sell, Sym, Symx };

// matrixFormat Ell (CsrMatrixWrapper.H:146-149): `width` = longest row; slot i of row r lives at i * stride + r.  map
// holds the CSR position of each slot (-1 = padding), so the values are refreshed from the freshly permuted CSR values
// whatever path produced them.
struct EllDev {
    DevBuf<int32_t> cols, map;
    DevBuf<double> vals;
    int32_t width = 0;
    int64_t stride = 0;
    bool ready = false;
    uint64_t epoch = 0;
    int build(const HostPattern &pat, Stager &stager, hipStream_t st);  // (pattern on the host)
    void release();
    void refresh(const double *csr_vals, hipStream_t st);
    double bytes(int32_t n_rows) const { return 12.0 * (double)width * (double)stride + 40.0 * (double)n_rows; }
    DevEll view(int32_t n_rows, bool stream) const;
};

// Half storage of a symmetric matrix on a banded pattern (SymLayout, host_matrix.hpp): what the Coo/Csr formats run on
// when compress_indices and symmetric_half are set, the lduMatrix has no `lower` and no same-rank (cyclic) interface, the
// device copy keeps the caller's numbering and the pattern qualifies.  map refreshes the planes from the CSR values.
struct SymDev {
    DevBuf<uint8_t> mask;
    DevBuf<int32_t> map, order;  // (order: band_block_order, may be empty)
    DevBuf<double> planes;
    int32_t nd = 0, d[4] = {0, 0, 0, 0};
    bool ready = false;
    uint64_t epoch = 0;
    int build(const SymLayout &L, int32_t n_rows, Stager &stager, hipStream_t st, Props &props);
    // mask and map from the device pattern for the distances sd (build_sym_on_device found them); *done stays false
    // when a row holds more entries than the distances allow
    int fill_on_device(int32_t n_rows, const int32_t *row_ptrs, const int32_t *cols, const SymDistances &sd,
                       int32_t *flags, hipStream_t st, bool *done);
    // the part of the set-up that does not depend on where mask and map were built
    int finish(int nd, const int32_t *d, int32_t n_rows, Stager &stager, hipStream_t st, Props &props);
    void release();
    void refresh(const double *csr_vals, hipStream_t st);
    double bytes(int32_t n_rows) const { return 8.0 * (double)planes.n + 41.0 * (double)n_rows; }
    DevSym view(int32_t n_rows, bool stream, bool band_order) const;
};

// Half storage with per-chunk distances and explicit exceptions (SymxLayout, host_matrix.hpp): symmetric matrices that
// are banded only locally (multi-block meshes, refinement shells) -- tried when the global half storage does not
// qualify.  The planes and the explicit entries are refreshed from the CSR values through their maps.
struct SymxDev {
    DevBuf<SymxChunk> chunks, chunks_general;  // (dispatch order: lean kernel's list, general one's)
    DevBuf<uint8_t> mask;
    DevBuf<int32_t> map, ex_rowptr, ex_cols, ex_map, ex_lrow;
    DevBuf<double> planes, ex_vals;
    bool fast = false;
    double matrix_bytes = 0.0;  // bytes one SpMV reads of this layout
    bool ready = false;
    uint64_t epoch = 0;
    int build(const HostPattern &pat, Stager &stager, hipStream_t st, Props &props);  // (pattern on the host)
    void release();
    void refresh(const double *csr_vals, hipStream_t st);
    double bytes(int32_t n_rows) const { return matrix_bytes + 41.0 * (double)n_rows; }
    DevSymx view(int32_t n_rows, bool stream, int32_t xcd_group) const;
};

// Device copy of an index-compressed chunked ELL (SellChunk, common.hpp; SellLayout, host_matrix.hpp) of some CSR
// matrix whose values live elsewhere: the system matrix (compress_indices) or ISAI's W and W^T.  Pattern once
// (`upload`), values by `refresh` from the CSR value array.
struct SellDev {
    DevBuf<SellChunk> chunks;
    DevBuf<int32_t> dict, map;
    DevBuf<uint8_t> codes;
    DevBuf<double> vals;
    // spill: tails of the rows longer than their chunk's cap (spill_chunks: the per-chunk ranges of spill_rows)
    DevBuf<int32_t> spill_rows, spill_ptrs, spill_cols, spill_map, spill_chunks;
    DevBuf<double> spill_vals;
    int32_t n_spill = 0;
    int64_t slots = 0, read_slots = 0;
    double matrix_bytes = 0.0;  // bytes one SpMV reads of this layout (decides the cache policy of its loads)
    bool irregular = false;     // chunks with 16-bit delta / 32-bit column codes (unstructured meshes)
    int64_t band_rows = 0;      // a banded pattern (1-byte codes throughout): the largest offset any chunk's table holds
    bool ready = false;  // false: the pattern does not qualify (or no layout was uploaded)
    bool tried = false;  // (system matrix: built or found not to qualify for the current pattern)
    uint64_t epoch = 0;
    // rows of each wavefront's window stored longest first (sort_windows; the kernel undoes it: DevSell::rmap)
    DevBuf<uint16_t> rmap;
    bool sorted = false;
    // W / W^T: the layout of a pattern without spill, optionally with sorted windows
    int build(ogl_label n_rows, const ogl_label *row_ptrs, const ogl_label *cols, Stager &stager, hipStream_t st,
              bool sort_windows = false);
    int upload(const SellLayout &L, Stager &stager, hipStream_t st);
    void release();
    void refresh(const double *csr_vals, hipStream_t st);
    double bytes(int32_t n_rows) const { return matrix_bytes + 40.0 * (double)n_rows; }
    DevSell view(int32_t n_rows, bool stream, int32_t xcd_group = 0, const DevBuf<int32_t> *block_order = nullptr) const;
};

// Packed columns for the CSR-stream kernel (Stream21Chunk, common.hpp), built from the device pattern for irregular
// patterns of >= SPMV_TUNE_MIN_ROWS rows when compress_indices is set.  The values stay the CSR array: nothing to refresh.
struct Stream21Dev {
    DevBuf<Stream21Chunk> chunks;
    DevBuf<uint4> codes;
    DevBuf<int32_t> far_idx, far_col;  // the chunks' entries outside their 2^21-column windows
    bool ready = false;  // false: not built, or a chunk's columns span 2^21 or more / too many entries are far
    bool tried = false;  // built or found not to qualify for the current pattern
    int build(int32_t n_rows, int32_t nnz, const int32_t *row_ptrs, const int32_t *cols, hipStream_t st, Props &props);
    void release();
    void refresh(const double *, hipStream_t) {}
    void view(DevCsr &A) const;  // the packed-column fields of the CSR-stream view
};

// The fp32 copy of the matrix that the inner solve of the mixed-precision mode runs on: an fp32
// twin of the half storage's planes when that is the in-loop layout -- it shares SymDev's mask, map and order -- and an
// fp32 value array beside the device CSR (sharing its row pointers and columns) for every other in-loop layout.
// Allocated at the first mixed solve and kept; refreshed from the CSR values under the values epoch by one kernel that
// also reports the first value that overflows binary32.  A solver with processor interfaces keeps the fp32 twin of the
// non-local coefficients (A32_nl) next to it: same epoch, same overflow word, positions counted behind the local ones.
struct Fp32Dev {
    DevBuf<float> planes, vals, nl_vals;
    bool half = false;     // which of the two is in use
    uint64_t pat_id = 0;   // the pattern the buffers were sized for
    uint64_t epoch = 0;    // 0: stale
    int ensure(bool half_storage, uint64_t pattern, size_t count, size_t nl_count, hipStream_t st);
    // map: SymDev::map (half storage) or nullptr (CSR values); bad: device word that receives the overflowing position
    // (a non-local coefficient: local_count() + its position)
    void refresh(const int32_t *map, const double *csr_vals, const double *nl_csr_vals, int32_t *bad, hipStream_t st);
    int64_t local_count() const { return half ? (int64_t)planes.n - 2 : (int64_t)vals.n; }
    const float *values() const { return half ? planes.p : vals.p; }
    void release();
};

}  // namespace ogl
