// solver.cpp -- see solver.hpp.  Citations: reference tree (hpsim/OGL @ 2024-10-16).
#include "solver_internal.hpp"

#include "setup_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <future>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <sched.h>
#include <mutex>
#include <thread>

using namespace ogl;


// ------------------------------------------------------------------------------------------
// Stager
// ------------------------------------------------------------------------------------------
// ---- the host side of a transfer: [caller's pageable array] <-> [pinned buffer], split over helper threads ----
namespace {
#if defined(__x86_64__)
// 32-byte non-temporal stores (AVX2, checked at run time: the library travels as generic x86-64 code); head and
// tail, or the whole range without AVX2 (and on any other host architecture), by memcpy
__attribute__((target("avx2"))) void stream_copy_avx2(char *d, const char *s, size_t len)
{
    const size_t head = std::min(len, (size_t)(-(uintptr_t)d & 31));
    if (head) std::memcpy(d, s, head);
    d += head;
    s += head;
    len -= head;
    size_t i = 0;
    for (; i + 128 <= len; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + i + 64));
        const __m256i e = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(d + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(d + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(d + i + 64), c);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(d + i + 96), e);
    }
    _mm_sfence();
    if (i < len) std::memcpy(d + i, s + i, len - i);
}
#endif
void stream_copy(void *d, const void *s, size_t len)
{
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2") && std::getenv("OGL_STAGE_PLAIN_STORES") == nullptr;
    if (avx2 && len >= 4096) {
        stream_copy_avx2(static_cast<char *>(d), static_cast<const char *>(s), len);
        return;
    }
#endif
    std::memcpy(d, s, len);
}
}  // namespace

// Persistent helpers: a copy is cut into one part per thread (the caller takes part 0); the helpers sleep on a
// condition variable between copies, so a refresh does not pay a thread start per buffer.
class ogl::CopyPool {
public:
    explicit CopyPool(int n_threads) : n_(std::max(1, n_threads))
    {
        // (binding the helpers to different L3 domains of the caller's socket was measured and changes nothing:
        //  46 GB/s either way on the 2 x EPYC 9575F hosts -- the copy is not what limits a transfer any more)
        for (int t = 1; t < n_; ++t) helpers_.emplace_back([this, t] { run(t); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &h : helpers_) h.join();
    }
    void copy(void *dst, const void *src, size_t len)
    {
        if (n_ == 1 || len < (size_t(1) << 20)) {
            stream_copy(dst, src, len);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            dst_ = static_cast<char *>(dst);
            src_ = static_cast<const char *>(src);
            len_ = len;
            part_ = ((len + n_ - 1) / n_ + 4095) / 4096 * 4096;
            pending_ = n_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        stream_copy(dst_, src_, std::min(part_, len_));
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
    }

private:
    void run(int t)
    {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> g(m_);
            cv_.wait(g, [&] { return quit_ || gen_ != seen; });
            if (quit_) return;
            seen = gen_;
            char *d = dst_;
            const char *s = src_;
            const size_t len = len_, part = part_;
            g.unlock();
            const size_t off = (size_t)t * part;
            if (off < len) stream_copy(d + off, s + off, std::min(part, len - off));
            g.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }
    int n_;
    std::vector<std::thread> helpers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    char *dst_ = nullptr;
    const char *src_ = nullptr;
    size_t len_ = 0, part_ = 0;
    int pending_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};

Stager::~Stager()
{
    delete pool_;
    for (int i = 0; i < NBUF; ++i) {
        ledger::pinned_free(pin_[i]);
        if (ev_[i]) ev_destroy(ev_[i]);
    }
}

int Stager::init(size_t chunk_bytes)
{
    if (chunk_) return OGL_OK;
    for (int i = 0; i < NBUF; ++i) {
        OGL_HIP_CHECK(ledger::pinned_malloc(&pin_[i], chunk_bytes));
        OGL_HIP_CHECK(ev_create(&ev_[i], hipEventDisableTiming));
    }
    chunk_ = chunk_bytes;
    const char *e = std::getenv("OGL_STAGE_THREADS");
    int n_threads = std::max(1, std::min(32, e ? atoi(e) : 8));
    // ... but no more than the CPUs this thread may run on: an MPI rank bound to one core (mpirun --bind-to core) hands
    // its one-CPU mask on to the helpers, and eight of them time-slicing that core copy no faster than the caller alone
    int allowed = (int)std::thread::hardware_concurrency();
    cpu_set_t mask;
    if (sched_getaffinity(0, sizeof(mask), &mask) == 0) allowed = CPU_COUNT(&mask);
    n_threads = std::min(n_threads, std::max(1, allowed));
    pool_ = new CopyPool(n_threads);
    return OGL_OK;
}

int Stager::h2d(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    for (size_t off = 0; off < bytes; off += chunk_) {
        const size_t len = std::min(chunk_, bytes - off);
        const int k = next_;
        next_ = (next_ + 1) % NBUF;
        if (busy_[k]) OGL_HIP_CHECK(hipEventSynchronize(ev_[k]));
        pool_->copy(pin_[k], s + off, len);  // the borrowed host array is free again after this
        OGL_HIP_CHECK(hipMemcpyAsync(d + off, pin_[k], len, hipMemcpyHostToDevice, st));
        OGL_HIP_CHECK(hipEventRecord(ev_[k], st));
        busy_[k] = true;
    }
    return OGL_OK;
}

int Stager::d2h(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    // up to NBUF - 1 device-to-pinned copies in flight while the oldest buffer is copied out to the caller
    struct Flight {
        int k;
        size_t off, len;
    };
    std::vector<Flight> fl;
    size_t head = 0, off = 0;
    while (off < bytes || head < fl.size()) {
        while (off < bytes && fl.size() - head < (size_t)NBUF - 1) {
            const size_t len = std::min(chunk_, bytes - off);
            const int k = next_;
            next_ = (next_ + 1) % NBUF;
            if (busy_[k]) OGL_HIP_CHECK(hipEventSynchronize(ev_[k]));
            OGL_HIP_CHECK(hipMemcpyAsync(pin_[k], s + off, len, hipMemcpyDeviceToHost, st));
            OGL_HIP_CHECK(hipEventRecord(ev_[k], st));
            busy_[k] = true;
            fl.push_back({k, off, len});
            off += len;
        }
        const Flight f = fl[head++];
        OGL_HIP_CHECK(hipEventSynchronize(ev_[f.k]));
        pool_->copy(d + f.off, pin_[f.k], f.len);
        busy_[f.k] = false;
    }
    return OGL_OK;
}

// ------------------------------------------------------------------------------------------
// registry / solver lifetime
// ------------------------------------------------------------------------------------------
ogl_registry::~ogl_registry()
{
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    solvers.clear();
    comm.reset();
    peer_close();
    cached_precond.release();
    if (comm_stream) {
        (void)hipStreamSynchronize(comm_stream);
        stream_destroy(comm_stream);
        ev_destroy(ev_packed);
        ev_destroy(ev_received);
    }
    if (own_stream && stream) stream_destroy(stream);
}

void ogl_solver::drop_cg_graph()
{
    if (cg_graph) {
        (void)hipGraphExecDestroy(cg_graph);
        ledger::destroyed(ledger::GRAPH_EXEC);
    }
    cg_graph = nullptr;
    cg_graph_key = 0;
}

ogl_solver::~ogl_solver()
{
    drop_cg_graph();
    ledger::pinned_free(h_scal);
    ledger::dev_free(lead_box);
    ledger::dev_free(held_z_box);
    ledger::dev_free(held_q_heads);
    mixed.release();
    proj.release();
    for (auto &e : poll_ev)
        if (e) ev_destroy(e);
    for (auto &e : prof_ev)
        if (e) ev_destroy(e);
    for (auto &e : chk_ev)
        if (e) ev_destroy(e);
}

double ogl_solver::knob_value(Knob k, double dflt) const
{
    auto it = props.find(knob_entry(k).name);
    return it == props.end() ? dflt : it->second;
}

// Every range check of a property: the keyword, the offending value, what is allowed.
int ogl_solver::check_knob(Knob k) const { return check_entry(knob_entry(k)); }

int ogl_solver::check_entry(const KnobEntry &e) const
{
    const KnobDomain &d = e.domain;
    const auto it = props.find(e.name);
    const double v = it == props.end() ? e.dflt.value : it->second;
    if (d.type == KnobDomain::None) return OGL_OK;
    if (d.type == KnobDomain::Open ? v > d.lo && v < d.hi : v >= d.lo && v <= d.hi && v == std::floor(v)) return OGL_OK;
    char range[64];
    std::snprintf(range, sizeof range, d.type == KnobDomain::Open ? "a number in (%g, %g)" : "a whole number in [%g, %g]", d.lo, d.hi);
    std::string allowed = d.type == KnobDomain::Flag ? "0 or 1" : range;
    if (d.type == KnobDomain::Choice) {  // the numbers with their words
        int n = 0;
        allowed = "one of 0 (";
        for (const char *p = d.words; *p; ++p)
            if (*p == '|') allowed += "), " + std::to_string(++n) + " (";
            else allowed += *p;
        allowed += ")";
    }
    return fail(OGL_ERR_INVALID, "%s %g is not %s", e.name, v, allowed.c_str());
}

// Size above which matrix data is streamed past the caches (STREAM instantiations, common.hpp).  The
// property `streamAboveBytes` / the environment variable OGL_STREAM_ABOVE_BYTES override the built-in
// threshold: 0 forces the STREAM kernels onto small systems, which is how the parity tests reach them.
double ogl_solver::stream_above_bytes() const
{
    static const double env_default = [] {
        const char *e = std::getenv("OGL_STREAM_ABOVE_BYTES");
        return e ? atof(e) : STREAM_MATRIX_ABOVE_BYTES;
    }();
    return knob<Knob::streamAboveBytes>(env_default);
}

// What a turn of this solver touches BESIDES the system matrix and GKOCG's five vectors (which the built-in threshold
// was measured with): the preconditioner's own matrices (ISAI: W and W^T, GISAI: W; block Jacobi: its blocks) and the
// further vectors of GKOBiCGStab / the Krylov basis of GKOGMRES.  All of it passes through the Infinity Cache once per
// turn, so it counts when the question is "does the turn's working set still live there" (property streamTurnSet 0:
// the matrix alone decides, as before round 5).
double ogl_solver::turn_extra_bytes() const
{
    if (knob<Knob::streamTurnSet>() == 0.0) return 0.0;
    const double N = (double)pat.n_rows, nnz = (double)pat.local_nnz;
    double extra = 0.0;
    if (cfg.preconditioner == OGL_PRECOND_ISAI) extra += 10.0 * (nnz + N);      // tril(A) twice, ~10 bytes per entry
    if (cfg.preconditioner == OGL_PRECOND_GISAI) extra += 10.0 * nnz;
    if (cfg.preconditioner == OGL_PRECOND_BJ && cfg.max_block_size > 1) extra += 8.0 * cfg.max_block_size * N;
    if (cfg.preconditioner == OGL_PRECOND_IC) extra += 24.0 * (nnz + N) / 2.0;  // L and L^T, 12 bytes per entry
    if (cfg.preconditioner == OGL_PRECOND_ILU || cfg.preconditioner == OGL_PRECOND_IRILU) extra += 12.0 * nnz;
    if (cfg.preconditioner == OGL_PRECOND_IRILU) extra += 16.0 * N;  // the sweeps' two iterates
    if ((cfg.preconditioner == OGL_PRECOND_IC || cfg.preconditioner == OGL_PRECOND_ILU ||
         cfg.preconditioner == OGL_PRECOND_IRILU) && pat.renumbered())
        extra += 8.0 * N;  // the vector in the caller's order
    // Multigrid: the coarse matrices (12 bytes per entry, about half the fine level's entries in all) and the fine level's
    // inverse diagonal, aggregates and three vectors
    if (cfg.preconditioner == OGL_PRECOND_MULTIGRID) extra += 6.0 * nnz + 36.0 * N;
    if (cfg.preconditioner == OGL_PRECOND_CHEBYSHEV) extra += 8.0 * N;  // 1 / d (the second iterate: the temporary below)
    if (cfg.preconditioner != OGL_PRECOND_NONE && !(cfg.preconditioner == OGL_PRECOND_BJ && cfg.max_block_size == 1))
        extra += 16.0 * N;                                                      // materialised z (and the ISAI temporary)
    if (cfg.solver == OGL_SOLVER_BICGSTAB) extra += 32.0 * N;
    if (cfg.solver == OGL_SOLVER_GMRES) extra += 8.0 * N * ((cfg.krylov_dim > 0 ? cfg.krylov_dim : 100) + 1 - 3);
    return extra;
}

// chunks per XCD group of the CSR-stream / compressed SpMV (DevCsr::xcd_group): property `xcdGroup`, else the
// environment's OGL_XCD_GROUP, else what the pattern's set-up chose (0 = the kernels' built-in 4)
int32_t ogl_solver::xcd_group() const
{
    static const int env_default = [] {
        const char *e = std::getenv("OGL_XCD_GROUP");
        return e ? atoi(e) : -1;
    }();
    const int v = (int)knob<Knob::xcdGroup>((double)env_default);
    return v >= 0 ? v : pat_xcd_group;
}

DevCsr ogl_solver::csr(bool packed) const
{
    DevCsr A;
    A.n_rows = pat.n_rows;
    A.nnz = pat.local_nnz;
    A.row_ptrs = d_row_ptrs.p;
    A.cols = d_cols.p;
    A.vals = d_vals.p;
    A.stream = streamed(12.0 * (double)pat.local_nnz + 44.0 * (double)pat.n_rows);
    A.xcd_group = xcd_group();
    A.lds_rounds = knob<Knob::spmvLdsRounds>() == 2.0 ? 2 : 1;
    if (d_band_order.n) {
        A.block_order = d_band_order.p;
        A.n_blocks = (int32_t)d_band_order.n;
    }
    if (packed) s21_dev.view(A);
    return A;
}

// ------------------------------------------------------------------------------------------
// Device set-up (setup_kernels.hip): the pattern of a field straight from the lduMatrix addressing, without
// the host holding its 12 bytes per entry.  `np` carries the small parts (build_host_pattern_meta); the
// arrays land in d_row_ptrs / d_cols / d_ldu_mapping / d_diag_pos (allocated by the caller).  *built stays
// false when the addressing is not conforming (a face with owner >= neighbour): the host algorithm, which
// follows the reference's segment order for such input, takes over.
// ------------------------------------------------------------------------------------------
int ogl_solver::build_pattern_on_device(const ogl_ldu_view &ldu, HostPattern &np, bool *built)
{
    *built = false;
    hipStream_t st = reg->stream;
    const int32_t N = np.n_rows, F = np.upper_nnz;
    if (N == 0) return OGL_OK;
    std::vector<ogl_label> ir, ic;
    if (np.local_iface_nnz) local_interface_entries(ldu, ir, ic);
    DevBuf<int32_t> addr, counts, tmp, flags, d_ir, d_ic;
    OGL_TRY(addr.alloc(2 * (size_t)F + 2, st));
    OGL_TRY(counts.alloc((size_t)N, st));
    OGL_TRY(tmp.alloc(scan_tmp_len(N), st));
    OGL_TRY(flags.alloc(PATTERN_FLAGS, st));
    if (F) {
        OGL_TRY(reg->stager.h2d(addr.p, ldu.lower_addr, (size_t)F * sizeof(int32_t), st));
        OGL_TRY(reg->stager.h2d(addr.p + F, ldu.upper_addr, (size_t)F * sizeof(int32_t), st));
    }
    if (!ir.empty()) {
        OGL_TRY(d_ir.alloc(ir.size(), st));
        OGL_TRY(d_ic.alloc(ic.size(), st));
        OGL_TRY(reg->stager.h2d(d_ir.p, ir.data(), ir.size() * sizeof(int32_t), st));
        OGL_TRY(reg->stager.h2d(d_ic.p, ic.data(), ic.size() * sizeof(int32_t), st));
    }
    PatternBuild b;
    b.n_rows = N;
    b.n_faces = F;
    b.n_iface = (int32_t)ir.size();
    b.symmetric = np.symmetric ? 1 : 0;
    b.lower_addr = addr.p;
    b.upper_addr = addr.p + F;
    b.if_rows = d_ir.p;
    b.if_cols = d_ic.p;
    b.row_ptrs = d_row_ptrs.p;
    b.cols = d_cols.p;
    b.ldu_mapping = d_ldu_mapping.p;
    b.diag_pos = d_diag_pos.p;
    b.counts = counts.p;
    b.scan_tmp = tmp.p;
    b.flags = flags.p;
    launch_build_pattern(st, b);
    int32_t hf[PATTERN_FLAGS] = {};
    OGL_HIP_CHECK(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    if (hf[PAT_FLAG_OUT_OF_RANGE]) return fail(OGL_ERR_INVALID, "a face addresses a cell outside [0,%d)", N);
    if (hf[PAT_FLAG_NONCONFORMING]) return OGL_OK;
    np.local_on_host = false;
    *built = true;
    return OGL_OK;
}

// cols / ldu_mapping / row_ptrs of a device-built pattern for the host code that wants them (numbering
// policy, compressed layout, Ell, block-Jacobi blocks, ISAI pattern, export): once, on demand
int ogl_solver::download_local_pattern(HostPattern &hp)
{
    if (hp.local_on_host) return OGL_OK;
    hipStream_t st = reg->stream;
    const size_t nnz = (size_t)hp.local_nnz;
    hp.row_ptrs.resize((size_t)hp.n_rows + 1);
    hp.cols.resize(nnz);
    hp.ldu_mapping.resize(nnz);
    hp.rows.clear();  // (row of entry k = the r with row_ptrs[r] <= k < row_ptrs[r + 1]; nobody here needs the array)
    OGL_TRY(reg->stager.d2h(hp.row_ptrs.data(), d_row_ptrs.p, hp.row_ptrs.size() * sizeof(int32_t), st));
    if (nnz) {
        OGL_TRY(reg->stager.d2h(hp.cols.data(), d_cols.p, nnz * sizeof(int32_t), st));
        OGL_TRY(reg->stager.d2h(hp.ldu_mapping.data(), d_ldu_mapping.p, nnz * sizeof(int32_t), st));
    }
    hp.local_on_host = true;
    return OGL_OK;
}

// Reverse Cuthill-McKee on the device, level by level (setup_kernels.hip): start node of every component by one
// breadth-first sweep (the node of smallest degree in its last level), then Cuthill-McKee from it -- children of a
// node by ascending (degree, index), a node belonging to the earliest parent of the level before.  The same
// order as rcm_order (tests/test_gpu_device_setup.py).  A level costs four small launches and one 4-byte
// read-back; graphs with very many components or levels (chains) are left to the host.
int ogl_solver::rcm_on_device(const HostPattern &hp, std::vector<ogl_label> &new_id)
{
    new_id.clear();
    hipStream_t st = reg->stream;
    const int32_t N = hp.n_rows;
    if (N < 2) return OGL_OK;
    constexpr int MAX_COMPONENTS = 64, MAX_LEVELS = 60000;
    DevBuf<int32_t> lvl, key, order, scratch, cnt, tmp, nid;
    DevBuf<unsigned long long> cell;
    OGL_TRY(lvl.alloc((size_t)N, st));
    OGL_TRY(key.alloc((size_t)N, st));
    OGL_TRY(order.alloc((size_t)N, st));
    OGL_TRY(scratch.alloc((size_t)N, st));
    OGL_TRY(cnt.alloc((size_t)N + 2, st));
    OGL_TRY(tmp.alloc(scan_tmp_len(N), st));
    OGL_TRY(nid.alloc((size_t)N, st));
    OGL_TRY(cell.alloc(4, st));
    RcmWork w;
    w.n_rows = N;
    w.row_ptrs = d_row_ptrs.p;
    w.cols = d_cols.p;
    w.lvl = lvl.p;
    w.key = key.p;
    w.order = order.p;
    w.scratch = scratch.p;
    w.cnt = cnt.p;
    w.scan_tmp = tmp.p;
    w.cell = cell.p;
    launch_rcm_init(st, w);
    int levels = 0;
    // breadth-first levels from list[begin] (already placed at `begin`); returns the end of the list and the
    // start of its last level
    auto run_levels = [&](int32_t *list, int32_t begin, bool by_degree, int32_t *last_begin, int32_t *end_out) -> int {
        int32_t b = begin, e = begin + 1, level = 0;
        for (;;) {
            launch_rcm_level(st, w, list, b, e, level, by_degree);
            int32_t total = 0;
            OGL_HIP_CHECK(hipMemcpyAsync(&total, cnt.p + (e - b), sizeof(int32_t), hipMemcpyDeviceToHost, st));
            OGL_HIP_CHECK(hipStreamSynchronize(st));
            if (total == 0) break;
            b = e;
            e += total;
            ++level;
            if (++levels > MAX_LEVELS) return 1;
            // thin levels for thousands of levels on end (a chain, a very long duct): a launch-bound crawl
            if (level > 2000 && (int64_t)(e - begin) < 64 * (int64_t)level) return 1;
        }
        *last_begin = b;
        *end_out = e;
        return OGL_OK;
    };
    int32_t filled = 0;
    for (int comp = 0; filled < N; ++comp) {
        if (comp >= MAX_COMPONENTS) return OGL_OK;  // (new_id stays empty: host)
        launch_rcm_find_seed(st, w);
        unsigned long long seed64 = 0;
        OGL_HIP_CHECK(hipMemcpyAsync(&seed64, cell.p, sizeof(seed64), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        if (seed64 >= (unsigned long long)N) return fail(OGL_ERR_STATE, "device RCM lost %d nodes", N - filled);
        const int32_t seed = (int32_t)seed64;
        int32_t rp2[2] = {0, 0};
        OGL_HIP_CHECK(hipMemcpy(rp2, d_row_ptrs.p + seed, sizeof(rp2), hipMemcpyDeviceToHost));
        int32_t start = seed;
        if (rp2[1] - rp2[0] > 1) {  // (isolated cells and chain ends are peripheral already)
            int32_t last_begin = 0, end = 0;
            launch_rcm_start(st, w, scratch.p, 0, seed, 0);
            const int rc = run_levels(scratch.p, 0, /*by_degree*/ false, &last_begin, &end);
            if (rc == 1) return OGL_OK;
            if (rc != OGL_OK) return rc;
            launch_rcm_far_node(st, w, scratch.p, last_begin, end);
            unsigned long long far = 0;
            OGL_HIP_CHECK(hipMemcpyAsync(&far, cell.p + 1, sizeof(far), hipMemcpyDeviceToHost, st));
            OGL_HIP_CHECK(hipStreamSynchronize(st));
            OGL_HIP_CHECK(hipMemcpy(&start, scratch.p + last_begin + (int32_t)(far & 0xffffffffu), sizeof(int32_t),
                                    hipMemcpyDeviceToHost));
            launch_rcm_reset(st, w, scratch.p, end);
        }
        int32_t last_begin = 0, end = 0;
        launch_rcm_start(st, w, order.p, filled, start, 0);
        const int rc = run_levels(order.p, filled, /*by_degree*/ true, &last_begin, &end);
        if (rc == 1) return OGL_OK;
        if (rc != OGL_OK) return rc;
        filled = end;
    }
    launch_rcm_finish(st, w, nid.p);
    new_id.resize((size_t)N);
    OGL_TRY(reg->stager.d2h(new_id.data(), nid.p, (size_t)N * sizeof(int32_t), st));
    OGL_HIP_CHECK(hipGetLastError());
    props["rcmLevels"] = (double)levels;
    return OGL_OK;
}

// The cells along a Hilbert curve through their centres (hilbert_order, host_matrix.cpp) on the device: bounding box on the
// host (one pass over 3 N doubles), keys + stable radix sort + inverse permutation on the device.  Same numbering as the host's.
int ogl_solver::curve_on_device(ogl_label n, const double *centres, std::vector<ogl_label> &new_id)
{
    new_id.clear();
    if (n < 2) return OGL_OK;
    hipStream_t st = reg->stream;
    double lo[3] = {centres[0], centres[1], centres[2]}, hi[3] = {centres[0], centres[1], centres[2]};
    for (ogl_label c = 0; c < n; ++c)
        for (int d = 0; d < 3; ++d) {
            lo[d] = std::min(lo[d], centres[3 * (size_t)c + d]);
            hi[d] = std::max(hi[d], centres[3 * (size_t)c + d]);
        }
    double ext = 0.0;
    for (int d = 0; d < 3; ++d) ext = std::max(ext, hi[d] - lo[d]);
    const double scale = ext > 0.0 ? 65535.0 / ext : 0.0;
    DevBuf<double> d_c;
    DevBuf<unsigned long long> keys, keys_out;
    DevBuf<int32_t> cells, cells_out, nid;
    DevBuf<unsigned char> temp;
    const size_t temp_bytes = hilbert_sort_temp_bytes(n);
    OGL_TRY(d_c.alloc(3 * (size_t)n, st));
    OGL_TRY(keys.alloc((size_t)n, st));
    OGL_TRY(keys_out.alloc((size_t)n, st));
    OGL_TRY(cells.alloc((size_t)n, st));
    OGL_TRY(cells_out.alloc((size_t)n, st));
    OGL_TRY(nid.alloc((size_t)n, st));
    OGL_TRY(temp.alloc(std::max<size_t>(temp_bytes, 16), st));
    OGL_TRY(reg->stager.h2d(d_c.p, centres, 3 * (size_t)n * sizeof(double), st));
    OGL_TRY(hilbert_order_device(st, n, d_c.p, lo, scale, keys.p, keys_out.p, cells.p, cells_out.p, temp.p, temp_bytes, nid.p));
    new_id.resize((size_t)n);
    OGL_TRY(reg->stager.d2h(new_id.data(), nid.p, (size_t)n * sizeof(int32_t), st));
    return OGL_OK;
}

// ... and the entries that would fall outside their chunk's window of packed columns along that curve (choose_numbering)
int ogl_solver::curve_far_on_device(const HostPattern &hp, const std::vector<ogl_label> &new_id,
                                    const std::vector<ogl_label> &old_of, int64_t &far)
{
    hipStream_t st = reg->stream;
    const int32_t N = hp.n_rows;
    DevBuf<int32_t> nid, old;
    DevBuf<unsigned long long> cnt;
    OGL_TRY(nid.alloc((size_t)N, st));
    OGL_TRY(old.alloc((size_t)N, st));
    OGL_TRY(cnt.alloc(1, st));  // (zero-filled)
    OGL_TRY(reg->stager.h2d(nid.p, new_id.data(), (size_t)N * sizeof(int32_t), st));
    OGL_TRY(reg->stager.h2d(old.p, old_of.data(), (size_t)N * sizeof(int32_t), st));
    launch_curve_far_count(st, N, d_row_ptrs.p, d_cols.p, nid.p, old.p, cnt.p);
    unsigned long long got = 0;
    OGL_TRY(reg->stager.d2h(&got, cnt.p, sizeof(got), st));
    far = (int64_t)got;
    return OGL_OK;
}

int ogl_solver::renumber_on_device(HostPattern &hp, const std::vector<ogl_label> &new_id)
{
    hipStream_t st = reg->stream;
    const int32_t N = hp.n_rows;
    const size_t nnz = (size_t)hp.local_nnz;
    DevBuf<int32_t> nid, old_of, rp2, cols2, map2, dpos2, tmp;
    OGL_TRY(nid.alloc((size_t)N, st));
    OGL_TRY(old_of.alloc((size_t)N, st));
    OGL_TRY(rp2.alloc((size_t)N + 1, st));
    OGL_TRY(cols2.alloc(nnz + NNZ_PAD, st));
    OGL_TRY(map2.alloc(nnz + NNZ_PAD, st));
    OGL_TRY(dpos2.alloc(std::max<size_t>(1, (size_t)N), st));
    OGL_TRY(tmp.alloc(scan_tmp_len(N), st));
    OGL_TRY(reg->stager.h2d(nid.p, new_id.data(), (size_t)N * sizeof(int32_t), st));
    RenumberWork w;
    w.n_rows = N;
    w.new_id = nid.p;
    w.row_ptrs = d_row_ptrs.p;
    w.cols = d_cols.p;
    w.map = d_ldu_mapping.p;
    w.old_of = old_of.p;
    w.row_ptrs_out = rp2.p;
    w.cols_out = cols2.p;
    w.map_out = map2.p;
    w.diag_pos_out = dpos2.p;
    w.scan_tmp = tmp.p;
    launch_renumber_pattern(st, w);
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    d_row_ptrs.swap(rp2);
    d_cols.swap(cols2);
    d_ldu_mapping.swap(map2);
    d_diag_pos.swap(dpos2);
    hp.local_on_host = false;  // the host arrays are in the old numbering: fetch the new ones
    return download_local_pattern(hp);
}

// Half storage from the device pattern (build_sym_layout's rules, host_matrix.cpp): the distances that occur,
// then mask and map per row.  *done stays false when the pattern does not qualify.
int ogl_solver::build_sym_on_device(const HostPattern &np, SymDistances *sd_out, bool *done)
{
    *done = false;
    hipStream_t st = reg->stream;
    const int32_t N = np.n_rows;
    if (N <= 0) return OGL_OK;
    DevBuf<int32_t> work;  // [table | flags]
    OGL_TRY(work.alloc(SYM_TABLE + SYM_FLAGS, st));
    int32_t init[SYM_TABLE + SYM_FLAGS];
    for (int j = 0; j < SYM_TABLE; ++j) init[j] = SYM_EMPTY;
    for (int j = 0; j < SYM_FLAGS; ++j) init[SYM_TABLE + j] = 0;
    OGL_HIP_CHECK(hipMemcpyAsync(work.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    launch_sym_distances(st, N, d_row_ptrs.p, d_cols.p, work.p, work.p + SYM_TABLE);
    int32_t got[SYM_TABLE + SYM_FLAGS];
    OGL_HIP_CHECK(hipMemcpyAsync(got, work.p, sizeof(got), hipMemcpyDeviceToHost, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    if (got[SYM_TABLE + SYM_FLAG_TOO_MANY] || got[SYM_TABLE + SYM_FLAG_UNSORTED_ROW]) return OGL_OK;
    int32_t dist[SYM_TABLE];
    int nd = 0;
    for (int j = 0; j < SYM_TABLE; ++j)
        if (got[j] != SYM_EMPTY) dist[nd++] = got[j];
    std::sort(dist, dist + nd);
    if (nd < 2 || nd > SYM_MAX_OFFSETS || dist[0] != 0 || dist[nd - 1] > INT32_MAX / 2) return OGL_OK;
    const int64_t nc = n_chunks(N);
    const double upper_entries = (double)N + (double)np.upper_nnz;  // diagonal + one entry per face
    if ((double)nd * (double)nc * CHUNK_ROWS > SYM_MAX_PADDING * upper_entries + 8.0 * CHUNK_ROWS) return OGL_OK;
    SymDistances sd{};
    sd.nd = nd;
    for (int j = 0; j < nd; ++j) sd.d[j] = dist[j];
    OGL_TRY(sym_dev.fill_on_device(N, d_row_ptrs.p, d_cols.p, sd, work.p + SYM_TABLE, st, done));
    *sd_out = sd;
    return OGL_OK;
}

// The band of the device CSR arrays: the largest distance column - row when the pattern holds at most SYM_TABLE distinct
// ones (a structured mesh in its own numbering), else 0.  One small kernel per pattern (k_sym_distances), cached.
int ogl_solver::csr_band(int64_t *band)
{
    if (csr_band_pat != pat_id) {
        hipStream_t st = reg->stream;
        csr_band_rows = 0;
        DevBuf<int32_t> work;  // [table | flags]
        OGL_TRY(work.alloc(SYM_TABLE + SYM_FLAGS, st));
        int32_t io[SYM_TABLE + SYM_FLAGS];
        for (int j = 0; j < SYM_TABLE; ++j) io[j] = SYM_EMPTY;
        for (int j = 0; j < SYM_FLAGS; ++j) io[SYM_TABLE + j] = 0;
        OGL_HIP_CHECK(hipMemcpyAsync(work.p, io, sizeof(io), hipMemcpyHostToDevice, st));
        launch_sym_distances(st, pat.n_rows, d_row_ptrs.p, d_cols.p, work.p, work.p + SYM_TABLE);
        OGL_HIP_CHECK(hipMemcpyAsync(io, work.p, sizeof(io), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_HIP_CHECK(hipGetLastError());
        if (!io[SYM_TABLE + SYM_FLAG_TOO_MANY])
            for (int j = 0; j < SYM_TABLE; ++j)
                if (io[j] != SYM_EMPTY) csr_band_rows = std::max<int64_t>(csr_band_rows, io[j]);
        csr_band_pat = pat_id;
    }
    *band = csr_band_rows;
    return OGL_OK;
}

// Once per sparsity pattern: the compressed layout of the system matrix, derived on the host (or taken from
// choose_numbering); sell_dev.map refreshes the values from the permuted CSR values on the device.
int ogl_solver::build_sell(SellLayout *pre, bool pre_qualifies)
{
    SellLayout own;
    if (!pre) {
        OGL_TRY(download_local_pattern(pat));
        pre_qualifies = pat.n_rows > 0 && build_sell_layout(pat.n_rows, pat.row_ptrs.data(), pat.cols.data(), own);
        pre = &own;
    }
    sell_dev.tried = true;
    sell_dev.ready = false;
    if (pat.n_rows == 0 || !pre_qualifies) return OGL_OK;
    const SellLayout &L = *pre;
    OGL_TRY(sell_dev.upload(L, reg->stager, reg->stream));
    props["sellSpilledEntries"] = (double)sell_dev.n_spill;
    props["sellMatrixBytes"] = sell_dev.matrix_bytes;
    props["sellReadSlots"] = (double)L.read_slots;
    props["sellAllocatedSlots"] = (double)L.n_slots;
    props["sellChunksDelta16"] = (double)L.n_delta16;
    props["sellChunksCol32"] = (double)L.n_col32;
    return OGL_OK;
}

DevHalo ogl_solver::halo() const
{
    DevHalo H;
    H.n_boundary_rows = (int32_t)boundary_rows.size();
    H.boundary_rows = d_boundary_rows.p;
    H.entry_ptrs = d_boundary_ptrs.p;
    H.cols = d_nl_cols.p;
    H.vals = d_nl_vals.p;
    H.n_send = (int32_t)pat.send_idxs.size();
    H.send_idxs = d_send_idxs.p;
    return H;
}

int ogl_solver::upload_vec(DevBuf<double> &dst, const double *src)
{
    const size_t n = (size_t)pat.n_rows;
    if (n == 0) return OGL_OK;
    if (!src) {
        OGL_HIP_CHECK(hipMemsetAsync(dst.p, 0, n * sizeof(double), reg->stream));
        return OGL_OK;
    }
    return upload_rows(dst.p, src);
}

int ogl_solver::upload_rows(double *dst, const double *src)
{
    const size_t bytes = (size_t)pat.n_rows * sizeof(double);
    if (!pat.renumbered()) return reg->stager.h2d(dst, src, bytes, reg->stream);
    OGL_TRY(reg->stager.h2d(d_perm_tmp.p, src, bytes, reg->stream));
    launch_permute_scatter(reg->stream, pat.n_rows, d_new_id.p, d_perm_tmp.p, dst);
    return OGL_OK;
}

int ogl_solver::download_rows(double *dst, const double *src)
{
    const size_t bytes = (size_t)pat.n_rows * sizeof(double);
    if (!pat.renumbered()) return reg->stager.d2h(dst, src, bytes, reg->stream);
    launch_permute_gather(reg->stream, pat.n_rows, d_new_id.p, src, d_perm_tmp.p);
    return reg->stager.d2h(dst, d_perm_tmp.p, bytes, reg->stream);
}


// Values of a layout are gathered from d_vals once per coefficient upload, when the layout is about to be timed or used.
void ogl_solver::refresh_values(SpmvLayout l)
{
    auto fresh = [&](auto &L) {
        if (L.ready && L.epoch != vals_epoch) {
            L.refresh(d_vals.p, reg->stream);
            L.epoch = vals_epoch;
        }
    };
    switch (l) {
    case SpmvLayout::Ell: fresh(ell_dev); break;
    case SpmvLayout::Sell: fresh(sell_dev); break;
    case SpmvLayout::Sym: fresh(sym_dev); break;
    case SpmvLayout::Symx: fresh(symx_dev); break;
    default: break;  // (the CSR-stream kernel reads d_vals itself)
    }
}

void ogl_solver::release_layout(SpmvLayout l)
{
    switch (l) {
    case SpmvLayout::Csr21: s21_dev.release(); break;
    case SpmvLayout::Ell: ell_dev.release(); break;
    case SpmvLayout::Sell: sell_dev.release(); break;
    case SpmvLayout::Sym: sym_dev.release(); break;
    case SpmvLayout::Symx: symx_dev.release(); break;
    default: break;
    }
}

// Which kernel runs the in-loop SpMV, measured once per pattern where that is a question: the candidates read the same
// matrix and give the same bits (y and the fused dot partials), so this is a speed choice only and ranks are free to
// differ.  Each candidate's best of TIMED launches after WARM ones, the candidates interleaved within each round; ties go
// to the later candidate, a `pin` among them wins whatever the timing says; the losers are released.  Work vectors p
// (input, zeroed: the time does not depend on the values) and q (output) are free between solves.
int ogl_solver::tune_spmv_layouts(const std::vector<SpmvLayout> &cand, const SpmvLayout *pin, SpmvLayout *winner)
{
    hipStream_t st = reg->stream;
    EventPair ev;
    OGL_HIP_CHECK(ev_create(&ev[0]));
    OGL_HIP_CHECK(ev_create(&ev[1]));
    OGL_HIP_CHECK(hipMemsetAsync(d_p.p, 0, ((size_t)pat.n_rows + 2) * sizeof(double), st));
    SpmvDots dots;
    dots.with = d_p.p;
    dots.part = d_part0.p;
    for (SpmvLayout c : cand) refresh_values(c);
    constexpr int WARM = 2, TIMED = 5;
    std::vector<float> best(cand.size(), 1e30f);
    for (int round = 0; round < WARM + TIMED; ++round)
        for (size_t i = 0; i < cand.size(); ++i) {
            OGL_HIP_CHECK(hipEventRecord(ev[0], st));
            spmv_on(cand[i], SPMV_PLAIN, d_p.p, nullptr, d_q.p, dots, nullptr);
            OGL_HIP_CHECK(hipEventRecord(ev[1], st));
            OGL_HIP_CHECK(hipEventSynchronize(ev[1]));
            float ms = 0;
            OGL_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            if (round >= WARM) best[i] = std::min(best[i], ms);
        }
    OGL_HIP_CHECK(hipGetLastError());
    size_t w = 0;
    for (size_t i = 1; i < cand.size(); ++i)
        if (best[i] <= best[w]) w = i;
    for (size_t i = 0; i < cand.size(); ++i) {
        if (pin && cand[i] == *pin) w = i;
        static const char *const name[] = {"Csr", "Csr21", "Ell", "Sell", "Sym", "Symx"};
        props[std::string("spmvTuned") + name[(int)cand[i]] + "Us"] = 1e3 * best[i];
    }
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < cand.size(); ++i)
        if (i != w) release_layout(cand[i]);  // (no refreshes, no memory for a layout of no use to this pattern)
    *winner = cand[w];
    return OGL_OK;
}

// The layout of the in-loop SpMV, once this call's layouts are built and timed: Ell when that is the format; else, with
// compress_indices, the first that is ready of the half storage, its per-chunk variant, the compressed copy and the packed
// columns (the timing has released the losers); else the CSR arrays.  Refreshes it, sets the workgroup order, and
// writes every property that describes it.
int ogl_solver::select_spmv_layout()
{
    using L = SpmvLayout;
    L l = L::Csr;
    if (cfg.matrix_format == OGL_FORMAT_ELL) l = L::Ell;
    else if (!cfg.compress_indices) l = L::Csr;
    else if (sym_dev.ready) l = L::Sym;
    else if (symx_dev.ready) l = L::Symx;
    else if (sell_dev.ready) l = L::Sell;
    else if (s21_dev.ready) l = L::Csr21;
    refresh_values(l);
    spmv_layout = l;
    {   // Band-aware workgroup order of the compressed / CSR-stream kernels (the half-storage kernels take theirs from
        // their own distances): the chunks of rows r and r +- band run on one XCD, so a strip of x is fetched into one L2
        // instead of three.  Full storage of the 216^3 box, STREAM instantiation: 128.2 -> 124.6 us (0.718 -> 0.739 of
        // peak); the plain CSR-stream kernel takes the same time either way (195.7 / 195.8 us) but fetches 14 % less over the
        // fabric (1.19 -> 1.02 x the model's bytes, profiles/r06_pmc_nocompress_summary.json), so it gets the order too.
        // Property spmvBandRows: the band in rows, 0 = off, -1 (default) = the largest offset of a banded pattern (the
        // compressed layout's tables; for the CSR arrays the distance table of the half-storage set-up, csr_band()).
        int64_t band = (int64_t)knob<Knob::spmvBandRows>();
        if (band < 0) {
            band = 0;
            if (l == L::Sell) band = sell_dev.band_rows;
            // (single rank: the order has not been run next to the halo waits of a multi-rank SpMV on the CSR arrays)
            if ((l == L::Csr || l == L::Csr21) && pat.n_rows >= SPMV_TUNE_MIN_ROWS && !reg->comm->multi())
                OGL_TRY(csr_band(&band));
        }
        if (band != band_order_rows) {
            d_band_order.release();
            band_order_rows = band;
            std::vector<int32_t> order;
            if (band > 0) band_block_order(pat.n_rows, band, order);
            if (!order.empty()) {
                OGL_TRY(d_band_order.alloc(order.size(), reg->stream));
                OGL_TRY(reg->stager.h2d(d_band_order.p, order.data(), order.size() * sizeof(int32_t), reg->stream));
            }
            drop_cg_graph();
        }
    }
    // which layout the in-loop SpMV runs on (SpmvLayout) and which instantiation of its kernel (what a profiler lists;
    // bench.py looks up exactly that one)
    props["spmvLayout"] = l == L::Csr ? 0.0 : l == L::Ell ? 1.0 : l == L::Csr21 ? 3.0 : 2.0;
    bool stream = false, fast = false;
    switch (l) {
    case L::Ell: stream = ell().stream; break;
    case L::Sym: {
        const DevSym S = sym();
        stream = S.stream;
        fast = S.nd >= 2 && S.d[1] == 1;
        for (int j = 2; j < S.nd; ++j) fast = fast && (S.d[j] % 2 == 0);
        props["spmvSymPlanes"] = (double)S.nd;
        break;
    }
    case L::Symx: stream = symx().stream, fast = symx().fast; break;
    case L::Sell: stream = sell().stream; break;
    default: stream = csr().stream;
    }
    set_knob<Knob::spmvStream>(stream ? 1.0 : 0.0);
    props["spmvSymFast"] = fast ? 1.0 : 0.0;
    return OGL_OK;
}

int ogl_solver::ensure_vectors()
{
    hipStream_t st = reg->stream;
    // +2 so that a trailing double2 access of the last (odd) row stays inside the allocation
    const size_t n = (size_t)pat.n_rows + 2;
    const size_t nc = (size_t)n_chunks(pat.n_rows) + 1;
    OGL_TRY(d_x.alloc(n, st));
    OGL_TRY(d_b.alloc(n, st));
    OGL_TRY(d_r.alloc(n, st));
    OGL_TRY(d_p.alloc(n, st));
    OGL_TRY(d_q.alloc(n, st));
    OGL_TRY(d_w.alloc(n, st));
    OGL_TRY(d_part0.alloc(nc, st));
    OGL_TRY(d_part1.alloc(nc, st));
    OGL_TRY(d_part2.alloc(nc, st));
    OGL_TRY(d_scal.alloc(2, st));  // (two slots: the fused-finaliser kernels of small systems ping-pong between them)
    if (!h_scal) {
        OGL_HIP_CHECK(ledger::pinned_malloc(reinterpret_cast<void **>(&h_scal), 2 * sizeof(DevScalars)));
        for (auto &e : poll_ev) OGL_HIP_CHECK(ev_create(&e, hipEventDisableTiming));
    }
    return OGL_OK;
}

bool ogl_solver::saw_addressing(const ogl_ldu_view &ldu) const
{
    if (seen_lower_addr != ldu.lower_addr || seen_upper_addr != ldu.upper_addr || seen_faces != ldu.n_faces ||
        (ogl_label)seen_iface_cells.size() != ldu.n_interfaces)
        return false;
    for (ogl_label i = 0; i < ldu.n_interfaces; ++i) {
        const SeenIface &a = seen_iface_cells[(size_t)i];
        const ogl_interface &b = ldu.interfaces[i];
        if (a.face_cells != b.face_cells || a.size != b.size || a.kind != b.kind || a.neighb_proc != b.neighb_proc ||
            a.neighb_patch != b.neighb_patch)
            return false;
    }
    return true;
}

// checksum over (at most) 4096 evenly spaced entries of each off-diagonal array plus their last ones (bit patterns):
// what ogl_solver_set_matrix_like compares before it trusts a donor's device copy
static uint64_t offdiag_sample(const double *upper, const double *lower, int64_t F)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const double *a, int64_t i) {
        uint64_t w;
        std::memcpy(&w, a + i, sizeof(w));
        h = (h ^ w) * 1099511628211ull;
    };
    if (F <= 0 || !upper) return h;
    const int64_t step = std::max<int64_t>(1, F / 4096);
    for (int64_t i = 0; i < F; i += step) {
        mix(upper, i);
        if (lower) mix(lower, i);
    }
    mix(upper, F - 1);
    if (lower) mix(lower, F - 1);
    return h;
}

// ------------------------------------------------------------------------------------------
// HostMatrixWrapper: pattern once, coefficients every call (HostMatrix.C:15-96)
// ------------------------------------------------------------------------------------------
int ogl_solver::set_matrix(const ogl_ldu_view &ldu)
{
    OGL_HIP_CHECK(hipSetDevice(reg->device));
    hipStream_t st = reg->stream;
    TraceRange trace("update_matrix", field);
    const double t0 = now_ms();
    // (what a later sibling may take over from THIS call is recorded at its successful end only: a call that fails part-way
    //  leaves nothing to be trusted)
    seen_lower_addr = seen_upper_addr = nullptr;
    seen_faces = -1;
    seen_iface_cells.clear();
    const bool try_sell = cfg.matrix_format != OGL_FORMAT_ELL && cfg.compress_indices;
    // ---- coefficients (update_local_matrix_data :592-705) ----
    // MatrixInitFunctor::update only overwrites the matrix values when updateSysMatrix is set
    // (CsrMatrixWrapper.H:259); the fresh coefficients have no other consumer, so the transfer
    // is skipped altogether in that case.
    auto upload_coefficients = [&]() -> int {
        const int32_t N = pat.n_rows, F = pat.upper_nnz;
        const size_t nnz = (size_t)pat.local_nnz;
        std::vector<double> iface;
        if (pat.local_iface_nnz) {
            iface.resize(pat.local_iface_nnz);
            collect_interface_coeffs(ldu, true, iface.data());
        }
        if (cfg.reorder_on_host) {  // :608-633, scaling applied by the host update functions
            offdiag_valid = false;  // (d_source is not filled on this path: nothing for a sibling to take)
            source_diag_valid = false;
            props["offDiagReused"] = 0.0;
            OGL_TRY(download_local_pattern(pat));
            std::vector<double> sorted(nnz);
            if (pat.local_iface_nnz) {
                if (pat.symmetric)
                    ogl_host_symmetric_update_w_interface(pat.local_nnz, N, F, pat.ldu_mapping.data(),
                                                          cfg.scaling, ldu.diag, ldu.upper,
                                                          iface.data(), sorted.data());
                else
                    ogl_host_non_symmetric_update_w_interface(
                        pat.local_nnz, N, F, pat.ldu_mapping.data(), cfg.scaling, ldu.diag,
                        ldu.upper, ldu.lower, iface.data(), sorted.data());
            } else if (pat.symmetric) {
                ogl_host_symmetric_update(pat.local_nnz, F, pat.ldu_mapping.data(), cfg.scaling,
                                          ldu.diag, ldu.upper, sorted.data());
            } else {
                ogl_host_non_symmetric_update(pat.local_nnz, F, pat.ldu_mapping.data(), cfg.scaling,
                                              ldu.diag, ldu.upper, ldu.lower, sorted.data());
            }
            OGL_TRY(reg->stager.h2d(d_vals.p, sorted.data(), nnz * sizeof(double), st));
        } else {  // :634-704 -- H2D into the unsorted slots, then the device permutation (K9)
            double *src = d_source.p;
            // (ogl_solver_set_matrix_like: a sibling component's device copy of the same upper / lower arrays)
            const ogl_solver *d = share_from;
            const uint64_t sum = offdiag_sample(ldu.upper, pat.symmetric ? nullptr : ldu.lower, F);
            const bool reuse = d && d->offdiag_valid && d->matrix_set && !d->cfg.reorder_on_host && d->have_pattern &&
                               d->pat.fingerprint == pat.fingerprint && d->pat.upper_nnz == F && d->pat.n_rows == N &&
                               d->pat.symmetric == pat.symmetric && d->offdiag_upper == ldu.upper &&
                               (pat.symmetric || d->offdiag_lower == ldu.lower) && d->offdiag_sum == sum && F > 0;
            if (reuse) {
                OGL_HIP_CHECK(hipMemcpyAsync(src, d->d_source.p, (size_t)F * (pat.symmetric ? 1 : 2) * sizeof(double),
                                             hipMemcpyDeviceToDevice, st));
            } else {
                OGL_TRY(reg->stager.h2d(src, ldu.upper, (size_t)F * sizeof(double), st));          // :644-650
                if (!pat.symmetric)
                    OGL_TRY(reg->stager.h2d(src + F, ldu.lower, (size_t)F * sizeof(double), st));  // :653-660
            }
            offdiag_upper = ldu.upper;
            offdiag_lower = pat.symmetric ? nullptr : ldu.lower;
            offdiag_sum = sum;
            offdiag_valid = true;
            props["offDiagReused"] = reuse ? 1.0 : 0.0;
            OGL_TRY(reg->stager.h2d(src + pat.diag_start(), ldu.diag, (size_t)N * sizeof(double),
                                    st));                                                     // :663-669
            if (pat.local_iface_nnz)
                OGL_TRY(reg->stager.h2d(src + pat.diag_start() + N, iface.data(),
                                        iface.size() * sizeof(double), st));                  // :672-682
            launch_gather_coeffs(st, pat.local_nnz, d_ldu_mapping.p, src, d_vals.p);          // :700-703
            source_diag_valid = true;  // (d_vals' diagonal = the N doubles at src + diag_start)
        }
        // ---- non-local coefficients (:708-732): tiny, permuted on the host ----
        if (pat.non_local_nnz) {
            std::vector<double> cc(pat.non_local_nnz);
            collect_interface_coeffs(ldu, false, cc.data());
            h_nl_vals.resize(pat.non_local_nnz);
            for (int32_t e = 0; e < pat.non_local_nnz; ++e) h_nl_vals[e] = cc[pat.nl_ldu_mapping[e]];
            OGL_TRY(reg->stager.h2d(d_nl_vals.p, h_nl_vals.data(),
                                    h_nl_vals.size() * sizeof(double), st));
        }
        matrix_set = true;
        ++vals_epoch;  // (every derived layout is stale: the SpMV reads the CSR arrays until select_spmv_layout)
        spmv_layout = SpmvLayout::Csr;
        return OGL_OK;
    };
    // Has the addressing changed?  Counts first (free); then the hash of every face and interface cell,
    // which runs on helper threads WHILE the coefficients of the (presumably unchanged) pattern are
    // staged to the device: the arrays have the right sizes either way, and if the hash disagrees the
    // pattern is rebuilt and the coefficients go up again.
    const bool try_sym = try_sell && cfg.symmetric_half;
    const bool config_same = have_pattern && pat_renumber_mode == cfg.renumber &&
                             !(cfg.renumber != 0 && pat_try_sell != try_sell) && pat_try_sym == try_sym;
    bool first = true, coefficients_done = false;
    int upload_rc = OGL_OK;  // (a failed speculative upload is reported after the ranks have agreed below)
    if (config_same && same_counts(ldu, pat)) {
        // (ogl_solver_set_matrix_like: the sibling hashed these very addressing arrays a moment ago -- same pointers, same
        //  counts -- and this field's pattern carries the fingerprint it found: the 240 MB are not read a second and
        //  third time per time step)
        const bool hashed_by_sibling = share_from && share_from->have_pattern &&
                                       share_from->pat.fingerprint == pat.fingerprint && share_from->saw_addressing(ldu);
        const uint64_t known = pat.fingerprint;
        auto fp = hashed_by_sibling ? std::async(std::launch::deferred, [known] { return known; })
                                    : std::async(std::launch::async, [&ldu] { return addressing_fingerprint(ldu); });
        int rc = OGL_OK;
        if (!matrix_set || cfg.update_sys_matrix || cfg.regenerate) {
            rc = upload_coefficients();
            coefficients_done = rc == OGL_OK;
        }
        first = fp.get() != pat.fingerprint;  // (joined before any return)
        upload_rc = rc;
    }
    if (reg->comm->multi()) {
        // a rebuild is collective once the peer mesh is up (setup_peer_halo): every rank rebuilds
        // when any rank's addressing changed
        OGL_TRY(d_flag.alloc(2, st));
        const double mine = first ? 1.0 : 0.0;
        double any = 0.0;
        OGL_HIP_CHECK(hipMemcpyAsync(d_flag.p, &mine, sizeof(double), hipMemcpyHostToDevice, st));
        OGL_TRY(reg->allreduce(d_flag.p, 1));
        OGL_HIP_CHECK(hipMemcpyAsync(&any, d_flag.p, sizeof(double), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        first = any != 0.0;
    }
    if (upload_rc != OGL_OK) return upload_rc;
    // a rebuild -- this rank's own or one another rank asked for -- re-creates the value arrays: whatever was
    // uploaded speculatively above is gone
    if (first) coefficients_done = false;
    if (first) {  // :79-87
        // Nothing of the old pattern survives from here on (the value arrays are re-created below before the new
        // pattern is validated): a failure inside this block must not leave the old fingerprint in charge of
        // buffers of another size, and a captured turn must not be replayed on the new layouts
        have_pattern = false;
        matrix_set = false;
        drop_cg_graph();
        spmv_layout = SpmvLayout::Csr;
        ell_dev.ready = sym_dev.ready = symx_dev.ready = sell_dev.ready = sell_dev.tried = false;
        s21_dev.release();
        s21_dev.tried = layout_tuned = false;
        HostPattern np;
        // Where the pattern is built: on the device from the face addressing (setup_kernels.hip), unless the
        // environment / property says otherwise or the addressing is not conforming; host_matrix.cpp then
        static const bool host_setup_env = std::getenv("OGL_HOST_SETUP") != nullptr;
        const bool device_setup = !host_setup_env && knob<Knob::deviceSetup>() != 0.0;
        OGL_TRY(build_host_pattern_meta(ldu, np, /*check_faces*/ !device_setup));
        // (the hash of the addressing runs on helper threads next to everything below; joined before any return)
        auto fp_new = std::async(std::launch::async, [&ldu] { return addressing_fingerprint(ldu); });
        const size_t nnz = (size_t)np.local_nnz;
        OGL_TRY(d_row_ptrs.alloc((size_t)np.n_rows + 1, st));
        OGL_TRY(d_cols.alloc(nnz + NNZ_PAD, st));
        OGL_TRY(d_vals.alloc(nnz + NNZ_PAD, st));
        OGL_TRY(d_ldu_mapping.alloc(nnz + NNZ_PAD, st));
        OGL_TRY(d_source.alloc((size_t)np.source_len() + NNZ_PAD, st));
        source_diag_valid = false;
        OGL_TRY(d_diag_pos.alloc(std::max<size_t>(1, (size_t)np.n_rows), st));
        bool built_on_device = false;
        if (device_setup) OGL_TRY(build_pattern_on_device(ldu, np, &built_on_device));
        if (!built_on_device) {
            if (device_setup)  // (non-conforming addressing: the device pass has checked the face range already)
                for (ogl_label f = 0; f < np.upper_nnz; ++f)
                    if (ldu.lower_addr[f] < 0 || ldu.lower_addr[f] >= np.n_rows || ldu.upper_addr[f] < 0 ||
                        ldu.upper_addr[f] >= np.n_rows)
                        return fail(OGL_ERR_INVALID, "face %d addresses a cell outside [0,%d)", f, np.n_rows);
            build_local_pattern(ldu, np);
        }
        set_knob<Knob::deviceSetup>(device_setup ? 1.0 : 0.0);
        props["patternBuiltOnDevice"] = built_on_device ? 1.0 : 0.0;
        // A symmetric lduMatrix without same-rank interfaces is tried on the half storage first (banded with
        // at most SYM_MAX_OFFSETS - 1 distances = a structured mesh, whose numbering the policy below would
        // keep anyway): everything stays on the device then
        SymDistances sym_dist{};
        bool sym_on_device = false, sym_tried = false, renumbered_on_device = false;
        // (symmetricHalfWhole_enable 0: an experiment switch -- the per-chunk variant on a pattern the whole-matrix one takes)
        const bool whole_sym = knob<Knob::symmetricHalfWhole_enable>() != 0.0;
        if (built_on_device && whole_sym && try_sym && np.symmetric && np.local_iface_nnz == 0 && cfg.renumber != 1) {
            sym_tried = true;
            OGL_TRY(build_sym_on_device(np, &sym_dist, &sym_on_device));
        }
        // numbering of the device copy (config `renumber`); the compressed layout the policy may
        // have derived on the way is kept for build_sell below
        SellLayout pre_sell;
        bool pre_built = false;
        RenumberReport rep;
        if (sym_on_device) {
            rep.ratio_natural = rep.ratio_used = -1.0;  // (not measured: the pattern never came to the host)
        } else {
            OGL_TRY(download_local_pattern(np));
            // with the pattern on the device the two heavy steps of a renumbering run there (same results)
            NumberingHooks hooks;
            if (built_on_device) {
                hooks.rcm = [&](const HostPattern &hp, std::vector<ogl_label> &nid) {
                    return rcm_on_device(hp, nid) == OGL_OK && !nid.empty();
                };
                hooks.renumber_local = [&](HostPattern &hp, const std::vector<ogl_label> &nid) {
                    renumbered_on_device = renumber_on_device(hp, nid) == OGL_OK;
                    return renumbered_on_device;
                };
            }
            // (cell centres, when the caller passes them: the Hilbert-curve candidate; property renumberCurve 0 = RCM only)
            if (ldu.cell_centres && knob<Knob::renumberCurve>() != 0.0) {
                hooks.centres = ldu.cell_centres;
                if (built_on_device && knob<Knob::curveOnDevice>() != 0.0) {
                    hooks.curve = [&](ogl_label n, const double *centres, std::vector<ogl_label> &nid) {
                        return curve_on_device(n, centres, nid) == OGL_OK && !nid.empty();
                    };
                    hooks.curve_far = [&](const HostPattern &hp, const std::vector<ogl_label> &nid,
                                          const std::vector<ogl_label> &old, int64_t &far) {
                        return curve_far_on_device(hp, nid, old, far) == OGL_OK;
                    };
                }
            }
            OGL_TRY(choose_numbering(np, cfg.renumber, try_sell, &pre_sell, &pre_built, rep, &hooks));
        }
        pat_renumber_mode = cfg.renumber;
        pat_try_sell = try_sell;
        pat_try_sym = try_sym;
        props["rowsSortedByLength"] = rep.sorted_by_length ? 1.0 : 0.0;
        props["gatherSlotSectorRatio"] = rep.slot_ratio;
        props["renumbered"] = rep.applied ? 1.0 : 0.0;
        props["gatherSectorRatioNatural"] = rep.ratio_natural;
        props["gatherSectorRatio"] = rep.ratio_used;
        props["gatherSectorRatioRcm"] = rep.ratio_rcm;
        props["gatherSectorRatioCurve"] = rep.ratio_curve;
        props["renumberedAlongCurve"] = rep.curve_used ? 1.0 : 0.0;
        props["curveFarEntries"] = (double)rep.curve_far_entries;
        np.fingerprint = fp_new.get();
        pat = std::move(np);
        have_pattern = true;
        static std::atomic<uint64_t> pattern_counter{0};  // registries may live on different threads
        pat_id = ++pattern_counter;
        matrix_set = false;
        d_band_order.release();  // (the band-aware workgroup order belongs to the pattern it was built for)
        band_order_rows = 0;
        x_resident = b_resident = false;
        props["renumberedOnDevice"] = renumbered_on_device ? 1.0 : 0.0;
        if (!built_on_device || (rep.applied && !renumbered_on_device)) {  // the device does not hold the pattern (in this numbering) yet
            OGL_TRY(reg->stager.h2d(d_row_ptrs.p, pat.row_ptrs.data(),
                                    pat.row_ptrs.size() * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_cols.p, pat.cols.data(), nnz * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_ldu_mapping.p, pat.ldu_mapping.data(), nnz * sizeof(int32_t), st));
            // Csr::extract_diagonal takes the first (i, i) entry of a row
            std::vector<int32_t> dpos((size_t)pat.n_rows, -1);
            for (int32_t r = 0; r < pat.n_rows; ++r)
                for (int32_t k = pat.row_ptrs[r]; k < pat.row_ptrs[r + 1]; ++k)
                    if (pat.cols[k] == r) {
                        dpos[(size_t)r] = k;
                        break;
                    }
            if (!dpos.empty())
                OGL_TRY(reg->stager.h2d(d_diag_pos.p, dpos.data(), dpos.size() * sizeof(int32_t), st));
        }

        // halo: rows owning non-local entries (row-sorted triplets -> one run per row)
        boundary_rows.clear();
        boundary_ptrs.clear();
        for (int32_t e = 0; e < pat.non_local_nnz; ++e) {
            if (e == 0 || pat.nl_rows[e] != pat.nl_rows[e - 1]) {
                boundary_rows.push_back(pat.nl_rows[e]);
                boundary_ptrs.push_back(e);
            }
        }
        boundary_ptrs.push_back(pat.non_local_nnz);
        const size_t hn = (size_t)pat.non_local_nnz;
        {  // chunks whose fused dot partials must be redone after the non-local part was added
            std::vector<int32_t> bc, bc_ptr;
            for (size_t i = 0; i < boundary_rows.size(); ++i) {
                const int32_t r = boundary_rows[i];
                if (bc.empty() || bc.back() != r / CHUNK_ROWS) {
                    bc.push_back(r / CHUNK_ROWS);
                    bc_ptr.push_back((int32_t)i);
                }
            }
            bc_ptr.push_back((int32_t)boundary_rows.size());
            n_boundary_chunks = (int32_t)bc.size();
            OGL_TRY(d_boundary_chunk_ptr.alloc(bc_ptr.size(), st));
            OGL_TRY(reg->stager.h2d(d_boundary_chunk_ptr.p, bc_ptr.data(), bc_ptr.size() * sizeof(int32_t), st));
            OGL_TRY(d_ticket.alloc(1, st));
            OGL_TRY(d_boundary_chunks.alloc(bc.size(), st));
            if (!bc.empty())
                OGL_TRY(reg->stager.h2d(d_boundary_chunks.p, bc.data(), bc.size() * sizeof(int32_t), st));
        }
        {   // per chunk: its boundary rows (HaloFused) and its send rows (HaloPutFused)
            const size_t nc1 = (size_t)n_chunks(pat.n_rows) + 1;
            std::vector<int32_t> bptr(nc1, 0), sptr(nc1, 0), spos(pat.send_idxs.size());
            for (int32_t r : boundary_rows) ++bptr[(size_t)(r / CHUNK_ROWS) + 1];
            for (int32_t r : pat.send_idxs) ++sptr[(size_t)(r / CHUNK_ROWS) + 1];
            n_put_chunks = 0;
            for (size_t c = 1; c < nc1; ++c) {
                if (sptr[c]) ++n_put_chunks;
                bptr[c] += bptr[c - 1];
                sptr[c] += sptr[c - 1];
            }
            std::vector<int32_t> fill(sptr.begin(), sptr.end() - 1);
            for (size_t j = 0; j < pat.send_idxs.size(); ++j)
                spos[(size_t)fill[(size_t)(pat.send_idxs[j] / CHUNK_ROWS)]++] = (int32_t)j;
            OGL_TRY(d_chunk_bptr.alloc(nc1, st));
            OGL_TRY(d_chunk_sptr.alloc(nc1, st));
            OGL_TRY(d_send_pos.alloc(std::max<size_t>(1, spos.size()), st));
            OGL_TRY(reg->stager.h2d(d_chunk_bptr.p, bptr.data(), nc1 * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_chunk_sptr.p, sptr.data(), nc1 * sizeof(int32_t), st));
            if (!spos.empty())
                OGL_TRY(reg->stager.h2d(d_send_pos.p, spos.data(), spos.size() * sizeof(int32_t), st));
        }
        OGL_TRY(d_boundary_rows.alloc(boundary_rows.size(), st));
        OGL_TRY(d_boundary_ptrs.alloc(boundary_ptrs.size(), st));
        OGL_TRY(d_nl_cols.alloc(hn, st));
        OGL_TRY(d_nl_vals.alloc(hn, st));
        OGL_TRY(d_send_idxs.alloc(pat.send_idxs.size(), st));
        OGL_TRY(d_send.alloc(pat.send_idxs.size(), st));
        OGL_TRY(d_recv.alloc(hn, st));
        if (hn) {
            OGL_TRY(reg->stager.h2d(d_boundary_rows.p, boundary_rows.data(),
                                    boundary_rows.size() * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_boundary_ptrs.p, boundary_ptrs.data(),
                                    boundary_ptrs.size() * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_nl_cols.p, pat.nl_cols.data(), hn * sizeof(int32_t), st));
            OGL_TRY(reg->stager.h2d(d_send_idxs.p, pat.send_idxs.data(),
                                    pat.send_idxs.size() * sizeof(int32_t), st));
        }
        neighbours.assign(pat.target_ids.begin(), pat.target_ids.end());
        counts.assign(pat.target_sizes.begin(), pat.target_sizes.end());
        if (!neighbours.empty() && !reg->comm->multi())
            return fail(OGL_ERR_STATE,
                        "matrix has processor interfaces but the registry has no communicator");
        // the receive side is assumed to mirror the send side (Partition.H:66-67)
        if ((size_t)pat.non_local_nnz != pat.send_idxs.size())
            return fail(OGL_ERR_INVALID, "send/receive sizes differ");
        OGL_TRY(ensure_vectors());
        if (pat.renumbered()) {
            OGL_TRY(d_new_id.alloc((size_t)pat.n_rows, st));
            OGL_TRY(d_perm_tmp.alloc((size_t)pat.n_rows + 2, st));
            OGL_TRY(reg->stager.h2d(d_new_id.p, pat.new_id.data(), (size_t)pat.n_rows * sizeof(int32_t), st));
            // (the inverse: block-Jacobi blocks stay those of the caller's numbering, generate_preconditioner)
            OGL_TRY(d_old_of.alloc((size_t)pat.n_rows, st));
            OGL_TRY(reg->stager.h2d(d_old_of.p, pat.old_of.data(), (size_t)pat.n_rows * sizeof(int32_t), st));
        }
        // a symmetric lduMatrix on a banded pattern keeps the OpenFOAM storage (diagonal + upper); the
        // compressed full-storage copy is then not built at all
        props["symmetricHalf"] = 0.0;
        bool sym_ok = false;
        if (sym_on_device) {
            OGL_TRY(sym_dev.finish(sym_dist.nd, sym_dist.d, pat.n_rows, reg->stager, st, props));
            sym_ok = true;
        } else if (!sym_tried && knob<Knob::symmetricHalfWhole_enable>() != 0.0 && try_sym && pat.symmetric &&
                   pat.local_iface_nnz == 0 && !pat.renumbered()) {
            SymLayout symL;
            if (build_sym_layout(pat.n_rows, pat.row_ptrs.data(), pat.cols.data(), symL)) {
                OGL_TRY(sym_dev.build(symL, pat.n_rows, reg->stager, st, props));
                sym_ok = true;
            }
        }
        props["symmetricHalfPerChunk"] = 0.0;
        if (!sym_ok && try_sym && pat.symmetric && pat.local_iface_nnz == 0 && !pat.renumbered() &&
            knob<Knob::symmetricHalfPerChunk_enable>() != 0.0) {
            // banded only locally (multi-block mesh, refinement shell): per-chunk distances + explicit exceptions
            OGL_TRY(download_local_pattern(pat));
            OGL_TRY(symx_dev.build(pat, reg->stager, st, props));
            if (symx_dev.ready) {
                sym_ok = true;
                props["symmetricHalfPerChunk"] = 1.0;
            }
        }
        if (!symx_dev.ready) symx_dev.release();
        if (sym_ok) {
            props["symmetricHalf"] = 1.0;
            // (per-chunk half storage of a system that is not launch-bound: timed once against the compressed full
            //  storage the numbering policy has laid out on the way, after the first values are in)
            if (symx_dev.ready && cfg.compress_indices == 1 && pat.n_rows >= SPMV_TUNE_MIN_ROWS) {
                OGL_TRY(pre_built ? build_sell(&pre_sell, rep.sell_used) : build_sell());
                props["sellMatrixBytes"] = symx_dev.matrix_bytes;
            }
            if (!sell_dev.ready) sell_dev.release();  // (nothing to time against when the compressed copy does not qualify)
        }
        if (!sym_dev.ready) sym_dev.release();
        if (!sym_dev.ready && !symx_dev.ready && pre_built && try_sell) OGL_TRY(build_sell(&pre_sell, rep.sell_used));
        OGL_TRY(setup_peer_halo());  // collective when the peer mesh is up (every rank, every pattern)
    }

    if (!coefficients_done && (!matrix_set || cfg.update_sys_matrix || cfg.regenerate)) OGL_TRY(upload_coefficients());
    if (cfg.matrix_format == OGL_FORMAT_ELL) {
        if (!ell_dev.ready) {
            OGL_TRY(download_local_pattern(pat));
            OGL_TRY(ell_dev.build(pat, reg->stager, st));
        }
    } else if (cfg.compress_indices && !sym_dev.ready && symx_dev.ready) {
        // per-chunk half storage built next to the compressed full storage (above): the faster one stays
        if (sell_dev.ready) {
            SpmvLayout win;
            OGL_TRY(tune_spmv_layouts({SpmvLayout::Sell, SpmvLayout::Symx}, nullptr, &win));
            if (win == SpmvLayout::Symx) {
                props["sellMatrixBytes"] = symx_dev.matrix_bytes;
            } else {
                props["symmetricHalf"] = 0.0;
                props["symmetricHalfPerChunk"] = 0.0;
                props["sellMatrixBytes"] = sell_dev.matrix_bytes;
            }
        }
    } else if (cfg.compress_indices && !sym_dev.ready) {
        if (!sell_dev.tried) OGL_TRY(build_sell());
        // irregular patterns (16 / 32-bit codes in the chunked ELL, or one that does not qualify for it at all: a
        // polyhedral mesh) of a size where the SpMV is not launch-bound: the CSR-stream kernel gets its packed
        // columns, and the candidates are timed once per pattern (compress_indices 2: no timing, the first that is
        // ready of the compressed copy and the packed columns runs)
        // (property spmvForceLayout 0 | 1 | 2: CSR-stream | compressed | packed columns whatever the timing says -- how
        //  the parity tests reach a layout on a pattern where another one wins.  A forced layout also counts below the
        //  tuning size, and 2 builds the packed columns next to a compressed copy of 8-bit codes: how those tests reach
        //  the packed columns on a system of a few rows)
        const int forced = (int)knob<Knob::spmvForceLayout>();
        const bool big = pat.n_rows >= SPMV_TUNE_MIN_ROWS || (forced >= 0 && forced < 3);
        const bool irregular_sell = sell_dev.ready && sell_dev.irregular;
        if (big && !s21_dev.tried && (irregular_sell || !sell_dev.ready || forced == 2))
            OGL_TRY(s21_dev.build(pat.n_rows, pat.local_nnz, d_row_ptrs.p, d_cols.p, st, props));
        if (big && cfg.compress_indices == 1 && !layout_tuned && (irregular_sell || s21_dev.ready)) {
            std::vector<SpmvLayout> cand{SpmvLayout::Csr};
            if (sell_dev.ready) cand.push_back(SpmvLayout::Sell);
            if (s21_dev.ready) cand.push_back(SpmvLayout::Csr21);
            const SpmvLayout by_force[3] = {SpmvLayout::Csr, SpmvLayout::Sell, SpmvLayout::Csr21};
            SpmvLayout win;
            OGL_TRY(tune_spmv_layouts(cand, forced >= 0 && forced < 3 ? &by_force[forced] : nullptr, &win));
            layout_tuned = true;
        }
    }
    OGL_TRY(select_spmv_layout());
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    // what this call's addressing arrays were (ogl_solver_set_matrix_like: a sibling built on the same arrays right after
    // need not hash them again)
    seen_lower_addr = ldu.lower_addr;
    seen_upper_addr = ldu.upper_addr;
    seen_faces = ldu.n_faces;
    seen_iface_cells.clear();
    for (ogl_label i = 0; i < ldu.n_interfaces; ++i) {
        const ogl_interface &f = ldu.interfaces[i];
        seen_iface_cells.push_back(SeenIface{f.face_cells, f.size, f.kind, f.neighb_proc, f.neighb_patch});
    }
    t_update_matrix_ms = now_ms() - t0;
    return OGL_OK;
}
