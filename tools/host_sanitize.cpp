// host_sanitize.cpp -- the host-side layout builders (per-chunk half storage, compressed chunked ELL), the numbering code and the
// preconditioners' pattern-only structures (counting transpose, ISAI row classes and scratch batches) on patterns read from files, meant for an AddressSanitizer / UBSan build (tests/test_cpp_host.py builds and runs it):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I ogl_amd/csrc tools/host_sanitize.cpp \
//       ogl_amd/csrc/host_matrix.cpp ogl_amd/csrc/common.cpp -lpthread -ldl -o host_sanitize && ./host_sanitize pattern.bin ...
// pattern.bin: int32 n_rows, int32 nnz, int32 row_ptrs[n_rows + 1], int32 cols[nnz]
#include <cstdio>
#include <cstdint>
#include <vector>
#include "ogl_amd.h"
#include "host_matrix.hpp"

// The shared counting transpose and build_isai_structure (host_matrix.hpp) on one pattern, spd and general, at
// sparsityPower 3 so that an unstructured mesh has rows beyond the wavefront limit.  The row classes are those of the
// generation kernels (32 / 64 / 2048 entries).  The scratch budget of 60,000 doubles is small enough that the huge rows
// of tests/test_cpp_host.py's octree and Voronoi patterns fall into several batches: their largest rows (printed as
// `max`) have 150 and 689 entries (general; 71 and 286 spd), i.e. systems of 22,500 and 474,721 doubles -- batches of a
// few rows on the octree, and rows that are a batch of their own above the budget on the Voronoi mesh.  Returns the
// number of violated properties.
static const int64_t ISAI_BUDGET = 60000;
static int check_isai(const char *name, int32_t n, const std::vector<int32_t> &rp, const std::vector<int32_t> &cols)
{
    using namespace ogl;
    int bad = 0;
    auto expect = [&](bool ok, const char *what) {
        if (!ok) {
            ++bad;
            printf("   isai FAILED %s: %s\n", name, what);
        }
    };
    HostPattern p;
    p.n_rows = n;
    p.local_nnz = (int32_t)cols.size();
    p.row_ptrs = rp;
    p.cols = cols;
    const IsaiRowClasses rc{32, 64, 2048};
    for (int spd = 0; spd < 2; ++spd) {
        IsaiStructure S;
        int32_t wide = -1;
        if (!build_isai_structure(p, spd != 0, 3, true, rc, ISAI_BUDGET, S, wide)) {
            printf("   isai %s: row %d beyond %d entries\n", spd ? "spd" : "general", wide, rc.max_row);
            continue;
        }
        // the transpose: map points at the source entry with (row, column) swapped; rows sorted; T(T(W)) = W
        std::vector<int32_t> trp, tc, tmap, back_rp, back_c, back_map;
        transpose_pattern(n, S.row_ptrs, S.cols, trp, tc, tmap);
        if (spd) expect(trp == S.t_row_ptrs && tc == S.t_cols && tmap == S.t_map, "W^T is the shared transpose of W");
        std::vector<int32_t> row_of(S.cols.size());
        for (int32_t r = 0; r < n; ++r)
            for (int32_t k = S.row_ptrs[r]; k < S.row_ptrs[r + 1]; ++k) row_of[k] = r;
        bool map_ok = trp.size() == (size_t)n + 1 && tc.size() == S.cols.size(), sorted = true;
        for (int32_t c = 0; map_ok && c < n; ++c)
            for (int32_t e = trp[c]; e < trp[c + 1]; ++e) {
                const int32_t k = tmap[e];
                map_ok = map_ok && k >= 0 && (size_t)k < S.cols.size() && S.cols[k] == c && row_of[k] == tc[e];
                sorted = sorted && (e == trp[c] || tc[e - 1] < tc[e]);
            }
        expect(map_ok, "every transposed entry maps to its source entry");
        expect(sorted, "transposed rows sorted by column");
        transpose_pattern(n, trp, tc, back_rp, back_c, back_map);
        expect(back_rp == S.row_ptrs && back_c == S.cols, "transpose of the transpose is the original");
        // wide / huge lists partition exactly the rows above the two thresholds
        std::vector<int32_t> w, h;
        int32_t max_row = 0;
        for (int32_t r = 0; r < n; ++r) {
            const int32_t len = S.row_ptrs[r + 1] - S.row_ptrs[r];
            max_row = len > max_row ? len : max_row;
            if (len > rc.wave_row) h.push_back(r);
            else if (len > rc.thread_row) w.push_back(r);
        }
        expect(w == S.wide_rows && h == S.huge_rows && max_row == S.max_row, "wide and huge rows partition the long rows");
        // batches: within the budget unless a single row; offsets of a batch tile [0, used) without overlap
        const std::vector<int32_t> &B = S.huge_batches;
        bool shape = !B.empty() && B.front() == 0 && B.back() == (int32_t)h.size() && S.huge_off.size() == h.size();
        bool fits = true, tiles = true;
        int64_t most = 0;
        for (size_t b = 0; shape && b + 1 < B.size(); ++b) {
            shape = shape && B[b] <= B[b + 1] && (B[b] < B[b + 1] || h.empty());
            int64_t used = 0;
            for (int32_t k = B[b]; k < B[b + 1]; ++k) {
                const int64_t len = S.row_ptrs[S.huge_rows[k] + 1] - S.row_ptrs[S.huge_rows[k]];
                tiles = tiles && S.huge_off[k] == used;
                used += len * len;
            }
            fits = fits && (used <= ISAI_BUDGET || B[b + 1] - B[b] == 1);
            most = used > most ? used : most;
        }
        expect(shape, "batches cover the huge rows in order");
        expect(fits, "every batch within the budget unless it is a single row");
        expect(tiles, "offsets within a batch do not overlap");
        expect(most == S.scratch_len, "scratch length is the largest batch");
        printf("   isai %s ok=%d max=%d wide=%zu huge=%zu batches=%zu\n", spd ? "spd" : "general", bad == 0, S.max_row,
               S.wide_rows.size(), S.huge_rows.size(), h.empty() ? (size_t)0 : B.size() - 1);
    }
    return bad;
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        FILE *f = fopen(argv[i], "rb");
        int32_t hdr[2];
        if (!f || fread(hdr, 4, 2, f) != 2) return 2;
        std::vector<int32_t> rp(hdr[0] + 1), cols(hdr[1]);
        if (fread(rp.data(), 4, rp.size(), f) != rp.size() || fread(cols.data(), 4, cols.size(), f) != cols.size()) return 3;
        fclose(f);
        int64_t st[8];
        int rc = ogl_host_symx_check(hdr[0], rp.data(), cols.data(), st);
        printf("%s symx rc=%d ok=%lld planar=%lld explicit=%lld fast=%lld general=%lld\n", argv[i], rc, (long long)st[0], (long long)st[2], (long long)st[3], (long long)st[6], (long long)st[7]);
        rc = ogl_host_sell_check(hdr[0], rp.data(), cols.data(), st);
        printf("   sell rc=%d ok=%lld\n", rc, (long long)st[0]);
        // the numbering candidates (reverse Cuthill-McKee, Hilbert curve through made-up centres) and the whole
        // renumbered pattern of the lduMatrix view that has this pattern (faces = its upper entries, owner-sorted)
        const int32_t n = hdr[0];
        std::vector<int32_t> nid(n > 0 ? n : 1);
        rc = ogl_host_rcm(n, rp.data(), cols.data(), nid.data());
        const double r_rcm = ogl_host_gather_sector_ratio(n, rp.data(), cols.data(), nid.data());
        std::vector<double> centres(3 * (size_t)(n > 0 ? n : 1));
        uint64_t lcg = 88172645463325252ull + (uint64_t)n;
        for (double &c : centres) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            c = (double)(lcg >> 11) / 9007199254740992.0;
        }
        const int rc_h = ogl_host_hilbert_order(n, centres.data(), nid.data());
        const double r_h = ogl_host_gather_sector_ratio(n, rp.data(), cols.data(), nid.data());
        std::vector<int32_t> lo, up;
        for (int32_t r = 0; r < n; ++r)
            for (int32_t e = rp[r]; e < rp[r + 1]; ++e)
                if (cols[e] > r) {
                    lo.push_back(r);
                    up.push_back(cols[e]);
                }
        std::vector<double> diag(n > 0 ? n : 1, 6.0), off(lo.size() + 1, -1.0);
        ogl_ldu_view v{};
        v.n_cells = n;
        v.n_faces = (int32_t)lo.size();
        v.lower_addr = lo.data();
        v.upper_addr = up.data();
        v.diag = diag.data();
        v.upper = off.data();
        v.cell_centres = centres.data();
        int renumbered = 0;
        for (int with_centres = 0; with_centres < 2; ++with_centres) {
            v.cell_centres = with_centres ? centres.data() : nullptr;
            ogl_matrix_dims d{};
            if (ogl_host_pattern_renumbered(&v, 1, 1, &d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr) < 0)
                return 4;
            std::vector<int32_t> a(d.local_nnz + 1), b(d.local_nnz + 1), c(d.local_nnz + 1), nl(1), ids(1), sz(1), snd(1);
            renumbered += ogl_host_pattern_renumbered(&v, 1, 1, &d, a.data(), b.data(), c.data(), nl.data(), nl.data(), nl.data(),
                                                      ids.data(), sz.data(), snd.data(), nid.data());
        }
        printf("   numbering rcm rc=%d ratio %.3f  hilbert rc=%d ratio %.3f  renumbered %d\n", rc, r_rcm, rc_h, r_h, renumbered);
        bad += check_isai(argv[i], n, rp, cols);
    }
    return bad ? 5 : 0;
}
