// spmv_layouts.cpp -- see spmv_layouts.hpp.
#include "spmv_layouts.hpp"

#include <algorithm>
#include <cstdlib>

namespace ogl {

// ---- Ell ----
int EllDev::build(const HostPattern &pat, Stager &stager, hipStream_t st)
{
    const int32_t N = pat.n_rows;
    int32_t w = 0;
    for (int32_t r = 0; r < N; ++r) w = std::max(w, pat.row_ptrs[r + 1] - pat.row_ptrs[r]);
    const int64_t s = ((int64_t)N + 1) / 2 * 2 + 2;  // even, and the pair load of the last row fits
    const size_t len = (size_t)w * (size_t)s;
    std::vector<int32_t> hc(len, -1), hm(len, -1);
    for (int32_t r = 0; r < N; ++r)
        for (int32_t k = pat.row_ptrs[r], i = 0; k < pat.row_ptrs[r + 1]; ++k, ++i) {
            hc[(size_t)i * s + r] = pat.cols[k];
            hm[(size_t)i * s + r] = k;
        }
    OGL_TRY(cols.alloc(len + 2, st));
    OGL_TRY(map.alloc(len + 2, st));
    OGL_TRY(vals.alloc(len + 2, st));
    OGL_TRY(stager.h2d(cols.p, hc.data(), len * sizeof(int32_t), st));
    OGL_TRY(stager.h2d(map.p, hm.data(), len * sizeof(int32_t), st));
    width = w;
    stride = s;
    ready = true;
    epoch = 0;
    return OGL_OK;
}

void EllDev::release()
{
    for (auto *b : {&cols, &map}) b->release();
    vals.release();
    ready = false;
}

void EllDev::refresh(const double *csr_vals, hipStream_t st)
{
    launch_gather_coeffs_masked(st, (int64_t)width * stride, map.p, csr_vals, vals.p);
}

DevEll EllDev::view(int32_t n_rows, bool stream) const
{
    DevEll E;
    E.n_rows = n_rows;
    E.width = width;
    E.stride = stride;
    E.cols = cols.p;
    E.vals = vals.p;
    E.stream = stream;
    return E;
}

// ---- half storage ----
int SymDev::build(const SymLayout &L, int32_t n_rows, Stager &stager, hipStream_t st, Props &props)
{
    OGL_TRY(mask.alloc(L.mask.size(), st));
    OGL_TRY(map.alloc(L.map.size(), st));
    OGL_TRY(planes.alloc(L.map.size(), st));
    OGL_TRY(stager.h2d(mask.p, L.mask.data(), L.mask.size(), st));
    OGL_TRY(stager.h2d(map.p, L.map.data(), L.map.size() * sizeof(int32_t), st));
    return finish(L.nd, L.d, n_rows, stager, st, props);
}

int SymDev::fill_on_device(int32_t n_rows, const int32_t *row_ptrs, const int32_t *cols, const SymDistances &sd,
                           int32_t *flags, hipStream_t st, bool *done)
{
    *done = false;
    const int64_t nc = n_chunks(n_rows);
    const size_t mask_len = (size_t)nc * CHUNK_ROWS + 16, map_len = (size_t)nc * sd.nd * CHUNK_ROWS + 2;
    OGL_TRY(mask.alloc(mask_len, st));
    OGL_TRY(map.alloc(map_len, st));
    OGL_TRY(planes.alloc(map_len, st));
    OGL_HIP_CHECK(hipMemsetAsync(mask.p, 0, mask_len, st));
    OGL_HIP_CHECK(hipMemsetAsync(map.p, 0xFF, map_len * sizeof(int32_t), st));
    OGL_HIP_CHECK(hipMemsetAsync(flags, 0, SYM_FLAGS * sizeof(int32_t), st));
    launch_sym_fill(st, n_rows, row_ptrs, cols, sd, mask.p, map.p, flags);
    int32_t got[SYM_FLAGS];
    OGL_HIP_CHECK(hipMemcpyAsync(got, flags, sizeof(got), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    *done = !got[SYM_FLAG_TOO_MANY];
    return OGL_OK;
}

int SymDev::finish(int n_d, const int32_t *dist, int32_t n_rows, Stager &stager, hipStream_t st, Props &props)
{
    nd = n_d;
    for (int j = 0; j < 4; ++j) d[j] = j < n_d ? dist[j] : 0;
    std::vector<int32_t> o;
    band_block_order(n_rows, dist[n_d - 1], o);
    order.release();
    if (!o.empty()) {
        OGL_TRY(order.alloc(o.size(), st));
        OGL_TRY(stager.h2d(order.p, o.data(), o.size() * sizeof(int32_t), st));
    }
    ready = true;
    epoch = 0;
    // bytes one SpMV reads of this layout (bench.py's moved-bytes model): planes + masks
    props["sellMatrixBytes"] = 8.0 * (double)(map.n - 2) + (double)(mask.n - 16);
    props["sellReadSlots"] = (double)(map.n - 2);
    props["sellAllocatedSlots"] = (double)(map.n - 2);
    props["sellChunksDelta16"] = 0.0;
    props["sellChunksCol32"] = 0.0;
    props["sellSpilledEntries"] = 0.0;
    return OGL_OK;
}

void SymDev::release()
{
    mask.release();
    for (auto *b : {&map, &order}) b->release();
    planes.release();
    ready = false;
}

void SymDev::refresh(const double *csr_vals, hipStream_t st)
{
    launch_gather_coeffs_masked(st, (int64_t)map.n - 2, map.p, csr_vals, planes.p);
}

DevSym SymDev::view(int32_t n_rows, bool stream, bool band_order) const
{
    DevSym S;
    S.n_rows = n_rows;
    S.nd = nd;
    for (int j = 0; j < 4; ++j) S.d[j] = d[j];
    S.mask = mask.p;
    S.planes = planes.p;
    S.stream = stream;
    if (order.n && band_order) {
        S.block_order = order.p;
        S.n_blocks = (int32_t)order.n;
    }
    return S;
}

// ---- half storage with per-chunk distances ----
int SymxDev::build(const HostPattern &pat, Stager &stager, hipStream_t st, Props &props)
{
    ready = false;
    SymxLayout L;
    if (pat.n_rows == 0 || !build_symx_layout(pat.n_rows, pat.row_ptrs.data(), pat.cols.data(), L)) return OGL_OK;
    const size_t nex = L.ex_cols.size();
    // headers in dispatch order, each naming its chunk (symx_block_order): the lean kernel's list, the general one's
    std::vector<SymxChunk> hdr_ord[2];
    int64_t general_chunks = 0;
    for (int g = 0; g < 2; ++g) {
        std::vector<int32_t> order;
        symx_block_order(L, g == 1, order);
        hdr_ord[g].resize(order.size());
        for (size_t b = 0; b < order.size(); ++b) {
            if (order[b] >= 0) hdr_ord[g][b] = L.chunks[(size_t)order[b]];
            else hdr_ord[g][b] = SymxChunk{};
            hdr_ord[g][b].chunk = order[b];
            if (g == 1 && order[b] >= 0) ++general_chunks;
        }
    }
    OGL_TRY(chunks.alloc(hdr_ord[0].size(), st));
    OGL_TRY(chunks_general.alloc(hdr_ord[1].size(), st));
    OGL_TRY(ex_lrow.alloc(nex + NNZ_PAD, st));
    OGL_TRY(mask.alloc(L.mask.size(), st));
    OGL_TRY(map.alloc(L.map.size(), st));
    OGL_TRY(planes.alloc(L.map.size(), st));
    OGL_TRY(ex_rowptr.alloc(std::max<size_t>(1, L.ex_rowptr.size()), st));
    OGL_TRY(ex_cols.alloc(nex + NNZ_PAD, st));
    OGL_TRY(ex_map.alloc(nex + NNZ_PAD, st));
    OGL_TRY(ex_vals.alloc(nex + NNZ_PAD, st));
    if (!hdr_ord[0].empty())
        OGL_TRY(stager.h2d(chunks.p, hdr_ord[0].data(), hdr_ord[0].size() * sizeof(SymxChunk), st));
    if (!hdr_ord[1].empty())
        OGL_TRY(stager.h2d(chunks_general.p, hdr_ord[1].data(), hdr_ord[1].size() * sizeof(SymxChunk), st));
    OGL_TRY(stager.h2d(mask.p, L.mask.data(), L.mask.size(), st));
    OGL_TRY(stager.h2d(map.p, L.map.data(), L.map.size() * sizeof(int32_t), st));
    if (!L.ex_rowptr.empty())
        OGL_TRY(stager.h2d(ex_rowptr.p, L.ex_rowptr.data(), L.ex_rowptr.size() * sizeof(int32_t), st));
    if (nex) {
        OGL_TRY(stager.h2d(ex_cols.p, L.ex_cols.data(), nex * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(ex_map.p, L.ex_map.data(), nex * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(ex_lrow.p, L.ex_lrow.data(), nex * sizeof(int32_t), st));
    }
    props["symxGeneralChunks"] = (double)general_chunks;
    ready = true;
    fast = L.all_fast;
    epoch = 0;
    // bytes one SpMV reads of this layout: planes, masks, headers, explicit entries (value + column + row) and their
    // row pointers
    matrix_bytes = 8.0 * (double)(L.map.size() - 2) + (double)(L.mask.size() - 16) + 96.0 * (double)L.chunks.size() +
                   16.0 * (double)nex + 4.0 * (double)L.ex_rowptr.size();
    props["sellMatrixBytes"] = matrix_bytes;
    props["sellReadSlots"] = (double)(L.map.size() - 2);
    props["sellAllocatedSlots"] = (double)(L.map.size() - 2);
    props["sellChunksDelta16"] = 0.0;
    props["sellChunksCol32"] = 0.0;
    props["sellSpilledEntries"] = 0.0;
    props["symxPlanarEntries"] = (double)L.planar;
    props["symxExplicitEntries"] = (double)nex;
    return OGL_OK;
}

void SymxDev::release()
{
    for (auto *b : {&chunks, &chunks_general}) b->release();
    mask.release();
    for (auto *b : {&map, &ex_rowptr, &ex_cols, &ex_map, &ex_lrow}) b->release();
    for (auto *b : {&planes, &ex_vals}) b->release();
    ready = false;
}

void SymxDev::refresh(const double *csr_vals, hipStream_t st)
{
    launch_gather_coeffs_masked(st, (int64_t)map.n - 2, map.p, csr_vals, planes.p);
    const int32_t nex = (int32_t)(ex_cols.n - NNZ_PAD);
    if (nex > 0) launch_gather_coeffs(st, nex, ex_map.p, csr_vals, ex_vals.p);
}

DevSymx SymxDev::view(int32_t n_rows, bool stream, int32_t xcd_group) const
{
    DevSymx S;
    S.n_rows = n_rows;
    S.chunks = chunks.p;
    S.mask = mask.p;
    S.planes = planes.p;
    S.ex_rowptr = ex_rowptr.p;
    S.ex_cols = ex_cols.p;
    S.ex_vals = ex_vals.p;
    S.stream = stream;
    S.fast = fast;
    S.n_blocks = (int32_t)chunks.n;
    S.chunks_general = chunks_general.p;
    S.n_blocks_general = (int32_t)chunks_general.n;
    S.ex_lrow = ex_lrow.p;
    S.xcd_group = xcd_group;
    return S;
}

// ---- index-compressed chunked ELL ----
int SellDev::build(ogl_label n_rows, const ogl_label *row_ptrs, const ogl_label *cols, Stager &stager,
                   hipStream_t st, bool sort_windows)
{
    ready = false;
    sorted = false;
    rmap.release();
    SellLayout L;
    if (n_rows == 0) return OGL_OK;
    if (!sort_windows) {
        if (!build_sell_layout(n_rows, row_ptrs, cols, L, /*allow_spill*/ false)) return OGL_OK;
    } else {
        // The rows of every wavefront's window (SELL_WAVE_ROWS rows) longest first, in a copy of the pattern that only
        // this layout sees: what choose_numbering does for the system matrix through the numbering itself is done here
        // with a slot order of the layout's own, undone by the kernel (DevSell::rmap) -- W in the CALLER's triangle on a
        // renumbered copy has rows of 1 .. 7 entries next to each other and does not qualify otherwise.
        const int64_t nc = n_chunks(n_rows);
        std::vector<ogl_label> order((size_t)nc * CHUNK_ROWS);
        for (size_t i = 0; i < order.size(); ++i) order[i] = (ogl_label)i;
        auto len = [&](ogl_label r) { return row_ptrs[r + 1] - row_ptrs[r]; };
        bool moved = false;
        for (ogl_label k0 = 0; k0 < n_rows; k0 += SELL_WAVE_ROWS) {
            const auto b = order.begin() + k0, e = order.begin() + std::min<int64_t>(n_rows, (int64_t)k0 + SELL_WAVE_ROWS);
            std::stable_sort(b, e, [&](ogl_label x, ogl_label y) { return len(x) > len(y); });
            for (auto it = b; it != e && !moved; ++it) moved = *it != k0 + (ogl_label)(it - b);
        }
        if (!moved) return OGL_OK;
        std::vector<ogl_label> prp((size_t)n_rows + 1, 0), pc((size_t)row_ptrs[n_rows]), at((size_t)row_ptrs[n_rows]);
        for (ogl_label sr = 0; sr < n_rows; ++sr) prp[(size_t)sr + 1] = prp[(size_t)sr] + len(order[(size_t)sr]);
        for (ogl_label sr = 0; sr < n_rows; ++sr) {
            const ogl_label r = order[(size_t)sr];
            for (ogl_label k = row_ptrs[r], q = prp[(size_t)sr]; k < row_ptrs[r + 1]; ++k, ++q) {
                pc[(size_t)q] = cols[k];
                at[(size_t)q] = k;
            }
        }
        if (!build_sell_layout(n_rows, prp.data(), pc.data(), L, /*allow_spill*/ false)) return OGL_OK;
        for (auto &m : L.map)
            if (m >= 0) m = at[(size_t)m];  // (values are gathered from the CSR values of the pattern itself)
        std::vector<uint16_t> rm(order.size());
        for (size_t i = 0; i < order.size(); ++i) rm[i] = (uint16_t)(order[i] - (ogl_label)(i / CHUNK_ROWS * CHUNK_ROWS));
        OGL_TRY(rmap.alloc(rm.size(), st));
        OGL_TRY(stager.h2d(rmap.p, rm.data(), rm.size() * sizeof(uint16_t), st));
        sorted = true;
    }
    return upload(L, stager, st);
}

// The layout (build_sell_layout) on the device; `map` refreshes the values from the CSR values.  (A layout without
// spill leaves the spill buffers of an earlier one alone: n_spill = 0 keeps them out of the view.)
int SellDev::upload(const SellLayout &L, Stager &stager, hipStream_t st)
{
    OGL_TRY(chunks.alloc(L.chunks.size(), st));
    OGL_TRY(dict.alloc(L.dict.size(), st));
    OGL_TRY(codes.alloc(L.codes.size(), st));
    OGL_TRY(map.alloc(L.map.size(), st));
    OGL_TRY(vals.alloc(L.map.size(), st));
    OGL_TRY(stager.h2d(chunks.p, L.chunks.data(), L.chunks.size() * sizeof(SellChunk), st));
    OGL_TRY(stager.h2d(dict.p, L.dict.data(), L.dict.size() * sizeof(int32_t), st));
    OGL_TRY(stager.h2d(codes.p, L.codes.data(), L.codes.size(), st));
    OGL_TRY(stager.h2d(map.p, L.map.data(), L.map.size() * sizeof(int32_t), st));
    // spill: tails of the rows longer than their chunk's cap (row-sorted), added by a second pass
    n_spill = (int32_t)L.spill_cols.size();
    if (n_spill) {
        OGL_TRY(spill_rows.alloc(L.spill_rows.size(), st));
        OGL_TRY(spill_ptrs.alloc(L.spill_ptrs.size(), st));
        OGL_TRY(spill_cols.alloc(L.spill_cols.size(), st));
        OGL_TRY(spill_map.alloc(L.spill_map.size() + NNZ_PAD, st));
        OGL_TRY(spill_vals.alloc(L.spill_cols.size() + NNZ_PAD, st));
        OGL_TRY(spill_chunks.alloc(L.spill_chunk_ptr.size(), st));
        OGL_TRY(stager.h2d(spill_rows.p, L.spill_rows.data(), L.spill_rows.size() * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(spill_ptrs.p, L.spill_ptrs.data(), L.spill_ptrs.size() * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(spill_cols.p, L.spill_cols.data(), L.spill_cols.size() * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(spill_map.p, L.spill_map.data(), L.spill_map.size() * sizeof(int32_t), st));
        OGL_TRY(stager.h2d(spill_chunks.p, L.spill_chunk_ptr.data(), L.spill_chunk_ptr.size() * sizeof(int32_t), st));
    }
    slots = L.n_slots;
    read_slots = L.read_slots;
    irregular = L.n_delta16 + L.n_col32 > 0;
    // a banded pattern: the band the workgroup order of the kernel is built for (ogl_solver::select_spmv_layout)
    band_rows = 0;
    if (!irregular)
        for (int32_t d : L.dict)
            if (d != SELL_PAD_OFFSET) band_rows = std::max<int64_t>(band_rows, std::abs((int64_t)d));
    // bytes one SpMV reads of this layout (bench.py's moved-bytes model): the value planes and codes
    // up to every wavefront's own width (planes beyond it are allocated, not read), headers, tables
    const double read_frac = L.n_slots ? (double)L.read_slots / (double)L.n_slots : 1.0;
    matrix_bytes = 8.0 * (double)L.read_slots + read_frac * (double)(L.codes.size() - 16) +
                   (double)(L.chunks.size() * sizeof(SellChunk)) + 4.0 * (double)L.dict.size() +
                   16.0 * (double)L.spill_cols.size();  // spilled entries: value + column + their share of row data
    ready = true;
    epoch = 0;
    return OGL_OK;
}

void SellDev::release()
{
    for (auto *b : {&dict, &map, &spill_rows, &spill_ptrs, &spill_cols, &spill_map, &spill_chunks}) b->release();
    chunks.release();
    codes.release();
    for (auto *b : {&vals, &spill_vals}) b->release();
    rmap.release();
    n_spill = 0;
    ready = sorted = false;
}

void SellDev::refresh(const double *csr_vals, hipStream_t st)
{
    if (!ready) return;
    launch_gather_sell(st, (int32_t)chunks.n, chunks.p, map.p, csr_vals, vals.p);
    if (n_spill) launch_gather_coeffs(st, n_spill, spill_map.p, csr_vals, spill_vals.p);
}

DevSell SellDev::view(int32_t n_rows, bool stream, int32_t xcd_group, const DevBuf<int32_t> *block_order) const
{
    DevSell S;
    S.n_rows = n_rows;
    S.chunks = chunks.p;
    S.dict = dict.p;
    S.codes = codes.p;
    S.vals = vals.p;
    S.rmap = sorted ? rmap.p : nullptr;
    S.stream = stream;
    S.xcd_group = xcd_group;
    if (block_order && block_order->n) {
        S.block_order = block_order->p;
        S.n_blocks = (int32_t)block_order->n;
    }
    if (n_spill) {
        S.spill_chunk_ptr = spill_chunks.p;
        S.spill_rows = spill_rows.p;
        S.spill_ptrs = spill_ptrs.p;
        S.spill_cols = spill_cols.p;
        S.spill_vals = spill_vals.p;
    }
    return S;
}

// ---- packed columns of the CSR-stream kernel ----
int Stream21Dev::build(int32_t N, int32_t nnz, const int32_t *row_ptrs, const int32_t *cols, hipStream_t st,
                       Props &props)
{
    tried = true;
    ready = false;
    const size_t nc = (size_t)n_chunks(N);
    if (N == 0) return OGL_OK;
    DevBuf<int32_t> words, tmp, flags, far;
    OGL_TRY(chunks.alloc(nc, st));
    OGL_TRY(words.alloc(nc + 1, st));
    OGL_TRY(far.alloc(nc + 1, st));
    OGL_TRY(tmp.alloc(scan_tmp_len((int64_t)nc), st));
    OGL_TRY(flags.alloc(1, st));
    Stream21Build b;
    b.n_rows = N;
    b.row_ptrs = row_ptrs;
    b.cols = cols;
    b.chunks = chunks.p;
    b.words = words.p;
    b.scan_tmp = tmp.p;
    b.flags = flags.p;
    b.far = far.p;
    launch_stream21_plan(st, b);
    int32_t total = 0, total_far = 0;
    OGL_HIP_CHECK(hipMemcpyAsync(&total, words.p + nc, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipMemcpyAsync(&total_far, far.p + nc, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    // (a pattern whose chunks reach far beyond their 2^21-column windows all over the place -- a random numbering of a
    //  large mesh -- is left to the plain CSR-stream kernel)
    if (total < 0 || total_far < 0 || (double)total_far > STREAM21_MAX_FAR * (double)nnz) {
        chunks.release();
        return OGL_OK;
    }
    OGL_TRY(codes.alloc((size_t)total + 1, st));
    OGL_TRY(far_idx.alloc((size_t)total_far + 1, st));
    OGL_TRY(far_col.alloc((size_t)total_far + 1, st));
    launch_stream21_fill(st, b, codes.p, far_idx.p, far_col.p);
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    ready = true;
    props["csr21FarEntries"] = (double)total_far;
    // bytes one SpMV reads of this layout: values + code words + row pointers + chunk headers (+ the far lists and the
    // values and x their entries read a second time)
    props["csr21MatrixBytes"] = 8.0 * (double)nnz + 16.0 * (double)total + 4.0 * ((double)N + 1.0) + 16.0 * (double)nc +
                                24.0 * (double)total_far;
    return OGL_OK;
}

void Stream21Dev::release()
{
    chunks.release();
    codes.release();
    for (auto *b : {&far_idx, &far_col}) b->release();
    ready = false;
}

void Stream21Dev::view(DevCsr &A) const
{
    if (!ready) return;
    A.chunks21 = chunks.p;
    A.codes21 = codes.p;
    A.far_idx21 = far_idx.p;
    A.far_col21 = far_col.p;
}

// ---- fp32 copy for the mixed-precision mode ----
int Fp32Dev::ensure(bool half_storage, uint64_t pattern, size_t count, size_t nl_count, hipStream_t st)
{
    DevBuf<float> &b = half_storage ? planes : vals;
    if (half != half_storage || pat_id != pattern || b.n != count || nl_vals.n != nl_count) epoch = 0;
    half = half_storage;
    pat_id = pattern;
    (half_storage ? vals : planes).release();
    if (nl_count == 0) nl_vals.release();
    else if (int rc = nl_vals.alloc(nl_count, st)) return rc;
    return b.alloc(count, st);
}

void Fp32Dev::refresh(const int32_t *map, const double *csr_vals, const double *nl_csr_vals, int32_t *bad, hipStream_t st)
{
    DevBuf<float> &b = half ? planes : vals;
    // (the planes carry two slots of padding behind the map's last entry, as SymDev::refresh knows)
    launch_mixed_refresh(st, local_count(), map, csr_vals, b.p, bad);
    if (nl_vals.n) launch_mixed_refresh(st, (int64_t)nl_vals.n, nullptr, nl_csr_vals, nl_vals.p, bad, local_count());
}

void Fp32Dev::release()
{
    planes.release();
    vals.release();
    nl_vals.release();
    epoch = 0;
}

}  // namespace ogl
