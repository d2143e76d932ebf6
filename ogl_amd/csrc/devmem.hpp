// devmem.hpp -- device buffers (DevBuf) and the pinned staging of host arrays (Stager): what every owner of device
// memory in the solver builds on.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "common.hpp"
#include "ledger.hpp"

namespace ogl {

#define OGL_HIP_CHECK(expr)                                                                \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return ::ogl::fail(OGL_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                \
                               hipGetErrorString(e_), __FILE__, __LINE__);                 \
    } while (0)
#define OGL_TRY(expr)                 \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != OGL_OK) return rc_; \
    } while (0)

// PersistentArray<T> (DevicePersistent/Array/Array.H:91-229): a named device array that lives as
// long as its registry.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;    // elements in use
    size_t cap = 0;  // elements allocated (>= n)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        ledger::dev_free(p);
        p = nullptr;
        n = cap = 0;
    }
    void swap(DevBuf &o)
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
    }
    // `count` elements, zero-filled when the size changes.  A block that is large enough (and not more than four times
    // too large) is kept: sizes that go back and forth from solve to solve -- the registry-wide preconditioner store
    // taking scalar Jacobi, blocks, W in turn (Preconditioner.H:357: one key for all fields), a residual history whose
    // length follows the adaptive evaluation frequency -- then cost no hipFree / hipMalloc pair per time step, and the
    // same pointers come back (a captured hipGraph stays valid).
    int alloc(size_t count, hipStream_t st)
    {
        if (count == n && p) return OGL_OK;
        if (p && count > 0 && count <= cap && count >= cap / 4) {
            OGL_HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(T), st));
            n = count;
            return OGL_OK;
        }
        release();
        if (count == 0) return OGL_OK;
        OGL_HIP_CHECK(ledger::dev_malloc(reinterpret_cast<void **>(&p), count * sizeof(T)));
        OGL_HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(T), st));
        n = cap = count;
        return OGL_OK;
    }
};

// Pinned double-buffered staging for pageable host arrays (K10/K12: "pinned async copies").
// Pageable host arrays <-> device through a ring of pinned buffers.  The copy between the caller's array and a
// pinned buffer is what limits a coefficient refresh (one core moves 10-25 GB/s, the PCIe 5 x16 link takes 55): it
// is split over a small pool of persistent helper threads (OGL_STAGE_THREADS, default 8) that store past the
// caches (non-temporal: the DMA engine -- or, coming down, the caller -- reads the data from DRAM anyway, and a
// plain store would first read the destination line), while the DMA of the previous buffers is in flight.
class CopyPool;
class Stager {
public:
    static constexpr int NBUF = 4;
    ~Stager();
    int init(size_t chunk_bytes);
    int h2d(void *dst, const void *src, size_t bytes, hipStream_t st);
    int d2h(void *dst, const void *src, size_t bytes, hipStream_t st);  // returns after completion

private:
    void *pin_[NBUF] = {};
    hipEvent_t ev_[NBUF] = {};
    bool busy_[NBUF] = {};
    size_t chunk_ = 0;
    int next_ = 0;
    CopyPool *pool_ = nullptr;
};

}  // namespace ogl
