// solver_internal.hpp -- what the translation units of the solver share besides solver.hpp: small helpers with internal
// linkage.  solver.cpp: registry, staging, layouts, HostMatrixWrapper (set_matrix); solver_transport.cpp: the peer mesh
// and the all-reduce; solver_precond.cpp: Preconditioner.H:353-431; solver_krylov.cpp: the distributed product, the
// finalisers and the Krylov drivers (lduLduBase.H:189-308).
#pragma once
#include <chrono>
#include <cstddef>

#include "solver.hpp"

namespace ogl {
namespace {

inline double now_ms()
{
    using clk = std::chrono::steady_clock;
    return std::chrono::duration<double, std::milli>(clk::now().time_since_epoch()).count();
}

inline double *sums_ptr(DevScalars *s)
{
    return reinterpret_cast<double *>(reinterpret_cast<char *>(s) + offsetof(DevScalars, sums));
}

struct EventPair {  // destroyed on every return path
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair()
    {
        for (auto &x : e)
            if (x) ev_destroy(x);
    }
    hipEvent_t &operator[](int i) { return e[i]; }
};

}  // namespace
}  // namespace ogl

// The three-way split of a finaliser over the transports, `launch()` enqueueing it with the arguments `a`: one launch
// that reduces and runs the logic; on the peer mesh the same with the all-reduce inside it (peer_next); on the other
// rungs a reducing launch, Comm::allreduce on the n_sums doubles it left at `sums`, a launch of the logic.
template <class Args, class Launch>
int ogl_solver::split_finaliser(Args &a, double *sums, int n_sums, Launch launch)
{
    a.peer = ogl::PeerArgs{};
    a.do_reduce = a.do_logic = 1;
    if (reg->comm->multi() && !reg->peer_ready) {
        a.do_logic = 0;
        launch();
        OGL_TRY(reg->comm->allreduce(sums, n_sums, reg->stream));
        a.do_reduce = 0;
        a.do_logic = 1;
        launch();
        return OGL_OK;
    }
    if (reg->comm->multi()) a.peer = reg->peer_next();
    launch();
    a.peer = ogl::PeerArgs{};
    return OGL_OK;
}
