// solver_krylov.cpp -- the distributed product, the finalisers and the Krylov drivers: plan, prepare, the turns of every
// solver x turn shape, the loop with its hipGraph replay, finish (lduLduBase.H:189-308; [UPSTREAM] step order: SURVEY 8 a19-a21).
// See solver.hpp, solver_internal.hpp.
#include "launch_key.hpp"
#include "solver_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ogl;

// ------------------------------------------------------------------------------------------
// distributed::Matrix::apply: y = A_local x (+ dot partials), then y += A_non_local recv
// ------------------------------------------------------------------------------------------
// arguments of the next SpMV's halo exchange for a producer kernel that puts the values itself (step_1x)
HaloPutFused ogl_solver::begin_halo_put()
{
    HaloPutFused put;
    if (!(pat.non_local_nnz > 0 && peer_halo) || knob<Knob::haloFused>() == 0.0 || peer_safe_wait())
        return put;
    cur_halo = next_exchange(sizeof(double));
    put.P = cur_halo;
    put.chunk_sptr = d_chunk_sptr.p;
    put.send_pos = d_send_pos.p;
    put.send_idxs = d_send_idxs.p;
    put.ticket = d_ticket.p;
    put.n_put_chunks = n_put_chunks;
    return put;
}

// what a kernel needs to wait for exchange `ph` and to add the non-local part itself
HaloFused ogl_solver::halo_fused_args(const PeerHalo &ph) const
{
    HaloFused hf;
    hf.chunk_bptr = d_chunk_bptr.p;
    hf.boundary_rows = d_boundary_rows.p;
    hf.entry_ptrs = d_boundary_ptrs.p;
    hf.cols = d_nl_cols.p;
    hf.vals = d_nl_vals.p;
    hf.recv = peer_recv<double>(ph.wait.seq);
    hf.wait = ph.wait;
    hf.s = d_scal.p;
    return hf;
}

void ogl_solver::spmv_on(SpmvLayout l, int mode, const double *x, const double *b, double *y, const SpmvDots &dots,
                         const DevScalars *gate, const HaloFused &hf)
{
    hipStream_t st = reg->stream;
    switch (l) {
    case SpmvLayout::Ell: launch_spmv_ell(st, ell(), mode, x, b, y, dots, gate, hf); break;
    case SpmvLayout::Sym: launch_spmv_sym(st, sym(), mode, x, b, y, dots, gate, hf); break;
    case SpmvLayout::Symx: launch_spmv_symx(st, symx(), mode, x, b, y, dots, gate, hf); break;
    case SpmvLayout::Sell: launch_spmv_sell(st, sell(), mode, x, b, y, dots, gate, hf); break;
    case SpmvLayout::Csr:
    case SpmvLayout::Csr21: launch_spmv(st, csr(l == SpmvLayout::Csr21), mode, x, b, y, dots, gate, hf); break;
    }
}

int ogl_solver::dist_spmv(int mode, const double *x, const double *b, double *y,
                          const SpmvDots &dots, const DevScalars *gate, bool prepacked)
{
    hipStream_t st = reg->stream;
    if (pat.non_local_nnz == 0) {
        spmv_on(spmv_layout, mode, x, b, y, dots, gate);
        return OGL_OK;
    }
    const HaloOwner own{gate, d_scal.p};
    // peer-put transport: by default the non-local part is added inside the local kernel (HaloFused) -- a
    // distributed SpMV is then 2 launches (pack + put + signal | local + wait + non-local), 1 when the producer
    // of x has put the values itself; property haloFused 0 keeps the separate finish kernel (A/B)
    // peerSafeWait 1 (ranks that SHARE a device; switched on by peer_connect itself when two ranks
    // report the same PCI bus id): no workgroup of the SpMV waits -- ONE workgroup of a
    // kernel of its own does, then the non-local part is added by kernels that find the values there.  Many waiting
    // workgroups of several ranks on one device can hold every slot the producers' put kernels need.
    if (peer_halo && !peer_safe_wait() && knob<Knob::haloFused>() != 0.0) {
        PeerHalo ph = cur_halo;
        if (!prepacked) {
            ph = next_exchange(sizeof(double));
            launch_pack_put_signal(st, halo(), ph, x, own, d_ticket.p);
        }
        spmv_on(spmv_layout, mode, x, b, y, dots, gate, halo_fused_args(ph));
        return OGL_OK;
    }
    PeerHalo ph;
    OGL_TRY(halo_begin(x, own, ph));
    spmv_on(spmv_layout, mode, x, b, y, dots, gate);
    return halo_end(mode, ph, d_nl_vals.p, y, dots, own);
}

int ogl_solver::finalize(int phase, FinArgs &a)
{
    auto launch = [&] { launch_finalize(reg->stream, phase, d_scal.p, a); };
    if (a.n_sums == 0) {  // nothing to reduce: scalar logic only (identical on every rank)
        a.do_reduce = 0;
        a.do_logic = 1;
        launch();
        return OGL_OK;
    }
    return split_finaliser(a, sums_ptr(d_scal.p), a.n_sums, launch);
}

// ------------------------------------------------------------------------------------------
// The Krylov drivers
// ------------------------------------------------------------------------------------------
// One driver for GKOCG, GKOBiCGStab and GKOGMRES: plan (which turn shape) -> prepare (criterion, buffers, norm factor,
// initial residual, the sums of turn 0) -> batches of turns with the stop flag polled one batch late -> finish (x,
// history, perf).  One member function per solver x turn shape (turn_*); what they share per solve lives in KrylovRun.
//
// GKOBiCGStab ([UPSTREAM] gko::solver::Bicgstab), per turn:
//   rho = rr.r, sum|r| -> check#1 -> p = r + (rho/prev_rho * alpha/omega)(p - omega v) -> y = M^-1 p
//   -> v = A y, beta = rr.v -> alpha = rho/beta, s = r - alpha v, sum|s| -> check#2 (x += alpha y
//   when it stops) -> z = M^-1 s -> t = A z, gamma = s.t, beta = t.t -> omega = gamma/beta,
//   x += alpha y + omega z, r = s - omega t.
// Two checks per turn: maxIter is doubled (StoppingCriterion.H:188) and the reported count halved
// (GKOBiCGStab.H:114).
struct ogl_solver::KrylovRun {
    hipStream_t st = nullptr;
    int n = 0, nc = 0;
    DevScalars *s = nullptr, *s2 = nullptr;
    DevScalars *slot_s[2] = {nullptr, nullptr};
    int cur = 0;  // the slot that holds the scalars after everything enqueued so far (folded GKOBiCGStab turn only)
    bool bicg = false, gmres = false, generic = false, multi = false;
    // turn shapes (see plan)
    bool fused = false, fused2 = false, merged = false, merged_halo = false, bicg_fold = false, gmres_fold = false;
    int m = 0;        // Krylov dimension of GKOGMRES
    int ortho = 0;    // GKOGMRES: 0 modified Gram-Schmidt, 1 | 2 classical Gram-Schmidt in block form, one | two rounds
    int64_t ldv = 0;  // leading dimension of the Krylov bases
    // basisPrecision single: the basis is stored as floats (d_Vf, leading dimension ldvf, every vector 16-byte aligned) and
    // the turn's working vector lives in nx_buf, fp64, not in a basis slot
    bool basis_single = false;
    int64_t ldvf = 0;
    double *nx_buf = nullptr;
    GmresBasis basis{};
    double n_global = 0.0;
    size_t n_halo = 0;
    double *p0 = nullptr, *p1 = nullptr, *ph = nullptr;  // p of even / odd turns (merged turn), old p at the halo columns
    double *z_kept = nullptr;  // z = r / d, left behind by step_2r_fin for the gathers
    LeadBox lead{};  // leader finalisation of the folded turn (box == nullptr: every workgroup reduces for itself)
    uint32_t lead_tag = 0;  // GKOGMRES: tag of the last leader launch (host-side sequence, from 1 per solve)
    DevCriterion crit{};
    bool is_final = false;
    int max_checks = 0, max_turns = 0;
    int prof_stride = 0, prof_cap = 0;
    hipEvent_t ev_chk[2] = {nullptr, nullptr};  // (the solver's own pair, created once: ogl_solver::chk_ev)
    double t_start = 0.0;
    FinArgs fg{}, chk{}, f1{}, f2{};  // GMRES finaliser arguments; the head-of-turn check; one / two partial arrays
    const double *beta_ptr = nullptr;
    double *gm = nullptr, *gm_y = nullptr;
    double *y = nullptr, *z = nullptr;  // BiCGStab: identity preconditioner -> y aliases p, z aliases s
    int enq = 0;                        // turns enqueued so far
    double *gm_h(int i, int j) const { return gm + (size_t)j * (m + 1) + i; }
    HeldZ hz{};  // the held-z turn: SpMV | k_cg_step2r1x (hz.grid == 0: the three-launch turn)
    bool held_z() const { return hz.grid > 0; }
    HeldQ hq{};  // the held-q turn: one launch (hq.on; needs the held-z turn's plan, which its profiled turns run)
    PRing ring{};  // three-launch leader turn with ring.k p buffers: x touched every ring.k-th turn (k_cg_step1x_fin)
    double *p_of_turn(int turn) const  // p that turn `turn` reads
    {
        if (ring.k > 0) return ring.b[turn % ring.k];
        return (merged && (turn & 1)) ? p1 : p0;
    }
    PRing ring_of_turn(int turn) const
    {
        PRing r = ring;
        r.phase = ring.k > 0 ? turn % ring.k : 0;
        return r;
    }
    double *p_halo_of_turn(int turn) const { return ph + (size_t)(turn & 1) * n_halo; }
    // scalar Jacobi: V_it is divided by its norm at the head of turn `it`, in the pass that applies the preconditioner
    bool gmres_scale_late() const { return gmres && !generic && has_diag; }
    bool has_diag = false;
    bool folded() const { return fused || bicg_fold; }  // the check of a turn runs at the head of the next kernel
};

int ogl_solver::run_cg(ogl_perf *perf) { return run_krylov(perf); }
int ogl_solver::run_bicgstab(ogl_perf *perf) { return run_krylov(perf); }

// Property orthoMethod: how GKOGMRES orthogonalises the new Krylov vector.  GKOCG and GKOBiCGStab
// have no such step and ignore the keyword.  The block form takes all sums of a round through one finaliser launch of its
// own, which has no all-reduce: with several ranks it is refused, not run on modified Gram-Schmidt in silence.
int ogl_solver::ortho_requested(int *method)
{
    *method = 0;
    if (cfg.solver != OGL_SOLVER_GMRES) return OGL_OK;
    OGL_TRY(check_knob(Knob::orthoMethod));
    const double v = knob<Knob::orthoMethod>();
    const int n_ranks = reg->comm ? reg->comm->n_ranks : 1;
    if (v != 0.0 && n_ranks > 1)
        return fail(OGL_ERR_UNSUPPORTED, "orthoMethod %s runs GKOGMRES on one rank: this registry has %d ranks",
                    v == 1.0 ? "cgs" : "cgs2", n_ranks);
    *method = (int)v;
    return OGL_OK;
}

// Property basisPrecision: how GKOGMRES stores its Krylov basis: 0 double, 1 single -- every store
// into the basis rounded to binary32, every operation on it in double.  It has kernels in block form only (orthoMethod
// cgs | cgs2); with mgs it is refused, not run on a double basis in silence.  GKOCG and GKOBiCGStab ignore the keyword.
int ogl_solver::basis_requested(bool *single)
{
    *single = false;
    if (cfg.solver != OGL_SOLVER_GMRES) return OGL_OK;
    OGL_TRY(check_knob(Knob::basisPrecision));
    const double v = knob<Knob::basisPrecision>();
    int ortho = 0;
    OGL_TRY(ortho_requested(&ortho));
    if (v == 1.0 && ortho == 0)
        return fail(OGL_ERR_UNSUPPORTED, "basisPrecision single needs orthoMethod cgs or cgs2: orthoMethod mgs has no kernels "
                    "for a basis stored in fp32");
    *single = v == 1.0;
    return OGL_OK;
}

int ogl_solver::run_krylov(ogl_perf *perf)
{
    bool mixed_on = false;  // (property mixedPrecision: solver_mixed.cpp)
    OGL_TRY(mixed_requested(&mixed_on));
    if (mixed_on) return run_mixed(perf);
    props["mixedPrecisionInUse"] = 0.0;
    KrylovRun k;
    OGL_TRY(krylov_plan(k));
    OGL_TRY(krylov_prepare(k));
    OGL_TRY(krylov_loop(k));
    return krylov_finish(k, perf);
}

// Which solver, which turn shape.
int ogl_solver::krylov_plan(KrylovRun &k)
{
    hipStream_t st = k.st = reg->stream;
    const int n = k.n = pat.n_rows;
    DevScalars *s = k.s = d_scal.p;
    const int nc = k.nc = (int)n_chunks(n);
    const bool bicg = k.bicg = cfg.solver == OGL_SOLVER_BICGSTAB;
    const bool gmres = k.gmres = cfg.solver == OGL_SOLVER_GMRES;
    // Ginkgo's default Krylov dimension is 100; the reference has no keyword for it
    // (GKOGMRES.H:46-63), `krylovDim` is this build's addition
    k.m = cfg.krylov_dim > 0 ? cfg.krylov_dim : 100;
    k.ldv = (int64_t)n + 2;
    // block Jacobi (maxBlockSize > 1): z = M^-1 r is materialised by its own kernel; the scalar
    // case stays fused into the step kernels
    const bool generic = k.generic = precond_data && precond_data->materialises_z();  // (every kind but scalar Jacobi)
    k.has_diag = precond != nullptr;
    const bool multi = k.multi = reg->comm->multi();
    const bool small = !multi && nc >= 1 &&
                       nc <= std::min((int)knob<Knob::fusedFinMaxChunks>(), FUSED_FIN_MAX_CHUNKS) &&
                       knob<Knob::fusedFinalizers>() != 0.0;
    // small single-rank GKOCG systems: finalisers folded into the step kernels, 3 launches per turn (kernels_krylov.hip)
    // ... and for LARGER single-rank GKOCG systems the same three launches with the LEADER finalisation (device_common.hpp):
    // workgroup 0 of the consuming kernel is the finaliser, the others poll its mailbox -- instead of two
    // single-workgroup launches (10 + 7 us at 10 M rows) and their dispatch gaps per turn (property leadFinalizers)
    const bool lead_any = !multi && !small && nc >= 3 * 16 && knob<Knob::leadFinalizers>() != 0.0;
    // (GKOCG with a materialised z -- block Jacobi, ISAI -- takes the leader finalisation too: the same two kernels with
    //  z in r's place, the preconditioner's launches between step_2r and the next turn's check)
    const bool lead_ok = lead_any && !bicg && !gmres;
    bool fused = k.fused = !bicg && !gmres && ((small && !generic) || lead_ok);
    k.lead = LeadBox{};
    k.s2 = s + 1;
    // ... and the same for small single-rank GKOBiCGStab systems: three finalisers folded into step_1 / step_2 / step_3
    // (k_bicg_fold1/2/3: 5 launches per turn instead of 8, plus the preconditioner's own)
    // (larger systems: the same five launches with the leader finalisation, any preconditioner -- the 2 M-row momentum
    //  systems of configs[2] spend a tenth of a turn in three single-workgroup launches and their gaps)
    k.bicg_fold = bicg && (small || lead_any) && knob<Knob::bicgFold>() != 0.0;
    // ... and for small single-rank GKOGMRES systems the finaliser between two Gram-Schmidt links is folded into the next
    // link's kernel (k_gmres_mgs_fold: one launch per link instead of two)
    // (larger systems: with the leader finalisation on request only, property gmresLead -- a Gram-Schmidt link moves 16 N
    //  bytes, and the wait for the leaders costs it what the finaliser launch did: 216^3 GMRES(30) 1068 against 1047 us per turn)
    OGL_TRY(ortho_requested(&k.ortho));  // (the block forms of Gram-Schmidt have no links to fold a finaliser into)
    props["orthoMethodInUse"] = (double)k.ortho;
    OGL_TRY(basis_requested(&k.basis_single));
    k.ldvf = ((int64_t)n + 3) & ~(int64_t)3;
    k.gmres_fold = gmres && !k.ortho && (small || (lead_any && knob<Knob::gmresLead>() != 0.0)) && knob<Knob::gmresFold>() != 0.0;
    // launches of a single-rank turn, averaged over a full cycle: the SpMV's one, the scaling's one and the Gram-Schmidt step
    // with the column's finaliser -- it + 3 folded links or 2 it + 4 launches at column `it`, 4 | 6 in block form (the
    // preconditioner's own launches, where it has any, are not counted)
    if (gmres)
        props["gmresLaunchesPerTurn"] =
            2.0 + (k.ortho ? 2.0 + 2.0 * k.ortho : k.gmres_fold ? 0.5 * (k.m - 1) + 3.0 : (double)(k.m - 1) + 4.0);
    k.slot_s[0] = s;
    k.slot_s[1] = k.s2;
    props["fusedFinalizersInUse"] = ((fused || k.bicg_fold || k.gmres_fold) && small) ? 1.0 : 0.0;
    // ... and on half storage step_1x(_fin) and the SpMV are one kernel (k_cg_turn_sym, k_cg_turn_sym_big): 2 launches
    // per turn for small systems, 4 for larger ones, p alternating between two buffers (single rank: with halos the
    // put and the wait for the neighbours' puts would sit in one kernel)
    // (larger systems, property fusedTurnBig: on while matrix and vectors live in the Infinity Cache -- 128^3 58.8 -> 54.7 us
    //  per turn, 136^3 66.3 -> 61.5 -- and off once they are streamed: 160^3 105.1 -> 104.5, 216^3 4149 -> 4190 turns/s,
    //  where the merged kernel runs 152 us for the 162 of step_1x + SpMV and step_2r pays 8 N more bytes for keeping z)
    // Several ranks (peer-put transport with the non-local part inside the local kernel): the same merge, 4 launches
    // per turn instead of 5 -- the neighbours' step_2r puts z of their send rows, this rank keeps the old p of its halo
    // columns and forms p_new there itself (kernels_spmv_sym.hip, k_cg_turn_sym_big<.., HALO>), so the merged kernel has
    // nothing to put and only waits for a put of the PREVIOUS launch.  Every rank must run the same turn (what the
    // neighbours put differs): agreed below together with the global row count.
    bool merged = !bicg && !gmres && !generic && nc >= 1 && spmv_layout == SpmvLayout::Sym &&
                  ((fused && small) ? knob<Knob::fusedTurn>() != 0.0 : knob<Knob::fusedTurnBig>(sym().stream ? 0.0 : 1.0) != 0.0);
    if (multi)
        merged = merged && peer_halo && knob<Knob::haloFused>() != 0.0 && knob<Knob::fusedTurnMulti>() != 0.0 &&
                 !peer_safe_wait();
    k.n_global = (double)n;
    if (multi) {
        // global row count (Partition.H:118-121) and the agreement on the turn, through the device all-reduce
        const double mine[2] = {(double)n, merged ? 0.0 : 1.0};
        double got[2] = {0.0, 0.0};
        OGL_HIP_CHECK(hipMemcpyAsync(sums_ptr(s), mine, sizeof(mine), hipMemcpyHostToDevice, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_TRY(reg->allreduce(sums_ptr(s), 2));
        OGL_HIP_CHECK(hipMemcpyAsync(got, sums_ptr(s), sizeof(got), hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        k.n_global = got[0];
        merged = got[1] == 0.0;
    }
    if ((lead_ok && fused) || (lead_any && (k.bicg_fold || k.gmres_fold))) {
        // (with the merged kernel two launches per turn, k_cg_turn_sym<.., LEAD> | k_cg_step2r_fin<LEAD>; that kernel has no
        //  streaming instantiation: the merge is on by default only where matrix and vectors live in the Infinity Cache)
        if (!lead_box) {
            void *b = nullptr;
            OGL_HIP_CHECK(ledger::dev_malloc(&b, LEAD_REPLICAS * LEAD_REPLICA_STRIDE * sizeof(unsigned long long), /*fine_grained=*/true));
            lead_box = static_cast<unsigned long long *>(b);
        }
        // (tags restart at 1 with every solve: no word of an earlier solve may survive)
        OGL_HIP_CHECK(hipMemsetAsync(lead_box, 0, LEAD_REPLICAS * LEAD_REPLICA_STRIDE * sizeof(unsigned long long), st));
        k.lead.box = lead_box;
        k.lead.timeout_ticks = (long long)(knob<Knob::leadTimeoutS>() * 1e8);
        k.lead.early_loads = knob<Knob::leadEarlyLoads>() != 0.0 ? 1 : 0;
    }
    props["leadFinalizersInUse"] = k.lead.box ? 1.0 : 0.0;
    props["fusedFinalizersInUse"] = ((fused || k.bicg_fold || k.gmres_fold) && small) ? 1.0 : 0.0;
    k.merged = merged;
    k.fused2 = fused && merged;
    k.merged_halo = merged && multi && pat.non_local_nnz > 0;  // (a rank without neighbours: the single-rank kernel)
    props["fusedTurnInUse"] = merged ? 1.0 : 0.0;
    return OGL_OK;
}

// Buffers, the stopping criterion, the norm factor, r = b - A x, and the sums the first check needs.
int ogl_solver::krylov_prepare(KrylovRun &k)
{
    hipStream_t st = k.st;
    const int n = k.n, nc = k.nc, m = k.m;
    DevScalars *s = k.s;
    const bool bicg = k.bicg, gmres = k.gmres, generic = k.generic, merged = k.merged;
    // (x every K-th turn: the leader turn of three launches -- not the merged kernel, which forms p_new at its gathers;
    //  property deferX = number of p buffers, 2 | 4 | 8, anything below 2 or deferX2 0: x every turn, p in place.  At 10 M
    //  rows two buffers give +1.2 % over none, four the same as two, eight lose 6 % -- the pending directions push the
    //  turn's other vectors out of the Infinity Cache: profiles/r06_defer_ab.txt)
    int ring_k = 0;
    if (k.lead.box != nullptr && k.fused && !k.fused2 && knob<Knob::deferX2>() != 0.0) {
        const double want = knob<Knob::deferX>();
        ring_k = want >= 8.0 ? 8 : want >= 4.0 ? 4 : want >= 2.0 ? 2 : 0;
    }
    props["deferXInUse"] = (double)ring_k;
    props["deferX2InUse"] = ring_k ? 1.0 : 0.0;
    if (merged || ring_k) OGL_TRY(d_p2.alloc((size_t)n + 2, st));
    for (int i = 2; i < ring_k; ++i) OGL_TRY(d_pring[i - 2].alloc((size_t)n + 2, st));
    if (merged && precond) OGL_TRY(d_z.alloc((size_t)n + 2, st));
    k.n_halo = (size_t)pat.non_local_nnz;
    if (k.merged_halo) {  // old p at the halo columns, two buffers like p itself; p = 0 before the first turn
        OGL_TRY(d_p_halo.alloc(2 * k.n_halo + 2, st));
        OGL_HIP_CHECK(hipMemsetAsync(d_p_halo.p, 0, d_p_halo.n * sizeof(double), st));
    }
    k.p0 = d_p.p;
    k.p1 = d_p2.p;
    k.ring.k = ring_k;
    for (int i = 0; i < ring_k; ++i) k.ring.b[i] = i == 0 ? d_p.p : i == 1 ? d_p2.p : d_pring[i - 2].p;
    k.ph = d_p_halo.p;
    k.z_kept = merged && precond ? d_z.p : nullptr;
    OGL_TRY(plan_held_z(k));

    // StoppingCriterion ctor + build_dist_stopping_criterion (StoppingCriterion.H:164-234)
    k.is_final = cfg.rel_tol == 0.0;  // get_is_final, :242
    const int prev_iters = (int)(k.is_final ? knob<Knob::prevSolveIters_final>() : knob<Knob::prevSolveIters>());
    const double prev_cost = knob<Knob::_prev_solve>();
    DevCriterion &crit = k.crit;
    crit.tolerance = cfg.tolerance;
    crit.rel_tol = cfg.rel_tol;
    crit.max_iter = bicg ? 2 * cfg.max_iter : cfg.max_iter;  // :188
    crit.export_res = cfg.export_res;
    ogl_host_adapt_criterion(&cfg, prev_iters, prev_cost, &crit.min_iter, &crit.frequency);
    if (crit.frequency < 1) return fail(OGL_ERR_INVALID, "evalFrequency must be >= 1");
    // the criterion stops at the first evaluated check at or after max(maxIter, minIter): checks
    // below minIter are skipped without a verdict (StoppingCriterion.C:77-81), so a minIter above
    // maxIter keeps the loop going, as in the reference
    k.max_checks = std::max(crit.max_iter, crit.min_iter) + crit.frequency + 1;
    k.max_turns = bicg ? k.max_checks / 2 + 1 : k.max_checks;  // CG and GMRES: one check per turn
    // (sized by what the keywords allow, not by this solve's adaptive frequency / minIter: the same block solve after solve)
    OGL_TRY(d_history.alloc((size_t)std::max(k.max_checks, crit.max_iter + std::max(1, cfg.norm_eval_limit) + 1) + 4, st));
    if (cfg.export_res)
        OGL_HIP_CHECK(hipMemsetAsync(d_history.p, 0, d_history.n * sizeof(double), st));
    if (k.bicg_fold) {  // (a folded kernel never writes a partial array it reads: six of them per turn)
        OGL_TRY(d_part3.alloc((size_t)nc, st));
        OGL_TRY(d_part4.alloc((size_t)nc, st));
        OGL_TRY(d_part5.alloc((size_t)nc, st));
    }
    if (bicg) {
        const size_t nv = (size_t)n + 2;
        OGL_TRY(d_v.alloc(nv, st));
        OGL_TRY(d_s.alloc(nv, st));
        OGL_TRY(d_t.alloc(nv, st));
        OGL_TRY(d_rr.alloc(nv, st));
        if (precond || generic) {
            OGL_TRY(d_y.alloc(nv, st));
            OGL_TRY(d_z.alloc(nv, st));
        }
    } else if (gmres) {
        // (only the basis of the precision this solve runs is sized; the other one, if an earlier solve left one, is kept)
        if (k.basis_single)
            OGL_TRY(d_Vf.alloc((size_t)(m + 1) * (size_t)k.ldvf, st));
        else
            OGL_TRY(d_V.alloc((size_t)(m + 1) * (size_t)k.ldv, st));
        k.nx_buf = d_q.p;  // (q is GKOCG's; here it is free once the norm factor is formed)
        k.basis.single = k.basis_single ? 1 : 0;
        k.basis.V = k.basis_single ? nullptr : d_V.p;
        k.basis.Vf = k.basis_single ? d_Vf.p : nullptr;
        k.basis.ld = k.basis_single ? k.ldvf : k.ldv;
        props["basisPrecisionInUse"] = k.basis_single ? 1.0 : 0.0;
        props["basisBytes"] = k.basis_single ? (double)(d_Vf.n * sizeof(float)) : (double)(d_V.n * sizeof(double));
        OGL_TRY(d_gm.alloc(gmres_state_len(m), st));
        OGL_HIP_CHECK(hipMemsetAsync(d_gm.p, 0, gmres_state_len(m) * sizeof(double), st));
        if (generic) OGL_TRY(d_z.alloc((size_t)n + 2, st));
        if (k.ortho) {
            OGL_TRY(d_gs_part.alloc((size_t)(m + 1) * (size_t)nc, st));
            OGL_TRY(d_gs_h.alloc((size_t)m + 1, st));
        }
    } else if (generic) {
        OGL_TRY(d_z.alloc((size_t)n + 2, st));
    }

    // profile_kernels = k > 0: every k-th turn's in-loop SpMV (the first of a BiCGStab turn) is bracketed by an event pair
    k.prof_stride = std::max(0, cfg.profile_kernels);
    k.prof_cap = k.prof_stride ? std::min((k.max_turns + k.prof_stride - 1) / k.prof_stride, 4096) : 0;
    while ((int)prof_ev.size() < 2 * k.prof_cap) {
        hipEvent_t e;
        OGL_HIP_CHECK(ev_create(&e));
        prof_ev.push_back(e);
    }
    for (int i = 0; i < 2; ++i) {  // (once per solver, not per solve: no runtime object comes and goes with a time step)
        if (!chk_ev[i]) OGL_HIP_CHECK(ev_create(&chk_ev[i]));
        k.ev_chk[i] = chk_ev[i];
    }

    k.t_start = now_ms();
    launch_reset_scalars(st, s, crit);
    proj_credit(st, s);  // (keyword guessProjectionCredit: what the first check's initial residual is counted from)

    FinArgs fa;
    // norm factor, part 1: xbar = mean(x) (StoppingCriterion.C:17-19)
    launch_partials_sum(st, n, d_x.p, d_part0.p);
    fa = FinArgs{};
    fa.part[0] = d_part0.p;
    fa.n_part = nc;
    fa.n_sums = 1;
    fa.n_local = (double)n;
    fa.n_global = k.n_global;  // (all-reduced in plan)
    OGL_TRY(finalize(FIN_MEAN, fa));
    // Axref = A * (xbar 1) (:24-29) into q
    launch_fill_xbar(st, n, d_w.p, s);
    OGL_TRY(dist_spmv(SPMV_PLAIN, d_w.p, nullptr, d_q.p, SpmvDots{}, nullptr));
    // r = b - A x  ([UPSTREAM] r = b; r = -1*A*x + 1*r)
    OGL_TRY(dist_spmv(SPMV_RESIDUAL, d_x.p, d_b.p, d_r.p, SpmvDots{}, nullptr));
    // norm factor, part 2 (:53-68)
    launch_partials_normfactor(st, n, d_b.p, d_q.p, d_r.p, d_part0.p);
    fa = FinArgs{};
    fa.part[0] = d_part0.p;
    fa.n_part = nc;
    fa.n_sums = 1;
    OGL_TRY(finalize(FIN_NORMFACTOR, fa));

    // solver initialisation + turn 0: rho, sum|r|, check (timed once as "time per residual norm
    // calculation", lduLduBase.H:287)
    OGL_HIP_CHECK(hipMemsetAsync(d_p.p, 0, (size_t)n * sizeof(double), st));
    k.fg = FinArgs{};
    k.fg.part[0] = d_part0.p;
    k.fg.part[1] = d_part1.p;
    k.fg.n_part = nc;
    k.fg.history = d_history.p;
    k.fg.gm = d_gm.p;
    k.fg.m = m;
    k.beta_ptr = reinterpret_cast<const double *>(reinterpret_cast<const char *>(s) + offsetof(DevScalars, beta));
    k.gm = d_gm.p;
    k.gm_y = d_gm.p + (size_t)(m + 1) * m + 2 * (size_t)m + (m + 1);
    if (gmres) {
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
        OGL_TRY(gmres_restart(k, nullptr));
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    } else if (bicg) {
        // rr = r ; p = v = 0 ([UPSTREAM] bicgstab::initialize); rho = rr.r = r.r
        OGL_HIP_CHECK(hipMemcpyAsync(d_rr.p, d_r.p, (size_t)n * sizeof(double),
                                     hipMemcpyDeviceToDevice, st));
        OGL_HIP_CHECK(hipMemsetAsync(d_v.p, 0, (size_t)n * sizeof(double), st));
        launch_cg_rho_norm(st, n, d_r.p, nullptr, d_part0.p, d_part1.p, s);
    } else {
        // p = q = 0 ([UPSTREAM] cg::initialize); z is never materialised (z = r * inv_diag on the fly)
        launch_cg_rho_norm(st, n, d_r.p, precond, d_part0.p, d_part1.p, s);
        if (k.z_kept) launch_mul(st, n, k.z_kept, d_r.p, precond, nullptr);  // (the z of the first k_cg_turn_sym)
        if (generic) {  // rho = r . (M^-1 r) with the block preconditioner
            apply_preconditioner(d_r.p, d_z.p, s, d_part0.p);
        }
    }
    k.chk = FinArgs{};
    k.chk.part[0] = d_part0.p;
    k.chk.part[1] = d_part1.p;
    k.chk.n_part = nc;
    k.chk.n_sums = 2;
    k.chk.history = d_history.p;
    if (!gmres && !k.folded()) {  // (folded turns: this check opens the first folded kernel)
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
        OGL_TRY(finalize(FIN_CG_CHECK, k.chk));
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    }
    if (k.merged_halo) {  // the z of the first merged turn (later ones: put by step_2r)
        cur_halo = next_exchange(sizeof(double));
        launch_pack_put_signal(st, halo(), cur_halo, k.z_kept ? k.z_kept : d_r.p, HaloOwner{s}, d_ticket.p);
    }

    k.f1 = FinArgs{};  // one partial array
    k.f1.part[0] = d_part0.p;
    k.f1.n_part = nc;
    k.f1.n_sums = 1;
    k.f1.history = d_history.p;
    k.f2 = k.f1;  // two partial arrays
    k.f2.part[1] = d_part1.p;
    k.f2.n_sums = 2;

    k.y = (precond || generic) ? d_y.p : d_p.p;  // identity: y aliases p, z aliases s
    k.z = (precond || generic) ? d_z.p : d_s.p;
    k.enq = 0;
    return OGL_OK;
}

// gmres::restart: rn = ||r||, rnc[0] = rn, V_0 = r / rn; the criterion keeps sum|r| of this r.  gate == nullptr: the
// restart before the first turn, whose finaliser runs the first check too.  With scalar Jacobi the division waits for the
// turn that follows (k_gmres_scale_mul).
int ogl_solver::gmres_restart(KrylovRun &k, const DevScalars *gate)
{
    launch_cg_rho_norm(k.st, k.n, d_r.p, nullptr, d_part0.p, d_part1.p, gate);  // r.r and sum|r|
    k.fg.n_sums = 2;
    k.fg.check_after = gate ? 0 : 1;
    OGL_TRY(finalize(FIN_GMRES_RESTART, k.fg));
    k.fg.check_after = 0;
    // (basisPrecision single: V_0 = fl32(r / rn) is stored by the head of the turn that follows)
    if (!k.basis_single && !k.gmres_scale_late()) launch_gmres_scale(k.st, k.n, d_V.p, d_r.p, k.beta_ptr, gate);
    return OGL_OK;
}

// solve_krylov + x += M^-1 (V y) over `cols` columns of the cycle
int ogl_solver::gmres_update_x(KrylovRun &k, int cols, const DevScalars *gate)
{
    if (cols <= 0) return OGL_OK;
    k.fg.n_sums = 0;
    k.fg.turn = cols;
    OGL_TRY(finalize(FIN_GMRES_SOLVE, k.fg));
    double *const before = k.generic ? d_w.p : nullptr;
    const double *const diag = k.generic ? nullptr : precond;
    if (k.basis_single)
        launch_gmres_update_x(k.st, k.n, d_Vf.p, k.ldvf, k.gm_y, cols, diag, d_x.p, before, gate);
    else
        launch_gmres_update_x(k.st, k.n, d_V.p, k.ldv, k.gm_y, cols, diag, d_x.p, before, gate);
    if (k.generic) {
        apply_preconditioner(d_w.p, d_z.p, gate);
        launch_add(k.st, k.n, d_x.p, d_z.p, gate);
    }
    return OGL_OK;
}

// ---- one turn of every solver x turn shape.  enq = index of the turn; pe >= 0: the event pair that brackets the turn's
// in-loop SpMV (profile_kernels), -1: none.  Kernels enqueued after the stop are no-ops (gated on the device scalars).

// GKOGMRES ([UPSTREAM] Gmres loop): check (on the residual of the last restart), restart when the cycle is full, then one
// Arnoldi step; gmres_fold: the finaliser between two Gram-Schmidt links runs inside the next link's kernel
int ogl_solver::turn_gmres(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n, m = k.m;
    const int64_t ldv = k.ldv;
    DevScalars *s = k.s;
    FinArgs &fg = k.fg;  // (the check at the head of this turn ran in the finaliser before it: restart or the last column's)
    if (enq > 0 && enq % m == 0) {
        OGL_TRY(gmres_update_x(k, m, s));
        OGL_TRY(dist_spmv(SPMV_RESIDUAL, d_x.p, d_b.p, d_r.p, SpmvDots{}, s));
        OGL_TRY(gmres_restart(k, s));
    }
    const int it = enq % m;
    if (k.basis_single) return turn_gmres_f32_basis(k, it, pe);
    double *v_it = d_V.p + (size_t)it * ldv, *nx = d_V.p + (size_t)(it + 1) * ldv;
    const double *w = v_it;  // identity preconditioner: w aliases V_it
    if (k.generic) {
        apply_preconditioner(v_it, d_w.p, s);
        w = d_w.p;
    } else if (precond) {  // V_it = (r | the last turn's new vector) / its norm, w = M^-1 V_it
        launch_gmres_scale_mul(st, n, v_it, it == 0 ? d_r.p : v_it, k.beta_ptr, precond, d_w.p, s);
        w = d_w.p;
    }
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, w, nullptr, nx, SpmvDots{}, s));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    // finish_arnoldi (modified Gram-Schmidt): H(k,it) = nx.V_k ; nx -= H(k,it) V_k
    fg.turn = it;
    fg.n_sums = 1;
    if (k.ortho) {
        // classical Gram-Schmidt in block form: every dot product of a round in one pass over the basis, every correction
        // in a second one; cgs2 runs a second round on the updated vector, whose dot products come out of the first
        // round's update pass, and H(j, it) is the sum of the two coefficients
        const int nv = it + 1;
        launch_gmres_multidot(st, n, nx, d_V.p, ldv, nv, d_gs_part.p, s);
        launch_gmres_fin_h(st, n, s, d_gs_part.p, nv, d_gs_h.p, k.gm_h(0, it), false);
        if (k.ortho == 2) {
            launch_gmres_block_update(st, n, nx, d_V.p, ldv, nv, d_gs_h.p, nullptr, d_gs_part.p, s);
            launch_gmres_fin_h(st, n, s, d_gs_part.p, nv, d_gs_h.p, k.gm_h(0, it), true);
        }
        launch_gmres_block_update(st, n, nx, d_V.p, ldv, nv, d_gs_h.p, d_part0.p, nullptr, s);
        fg.check_after = 1;
        OGL_TRY(finalize(FIN_GMRES_COL, fg));  // ||nx||, Givens, residual-norm recurrence, the next turn's check
        fg.check_after = 0;
    } else if (k.gmres_fold) {
        double *pin = d_part1.p, *pout = d_part0.p;  // (a link reads the partials of the one before it)
        for (int j = 0; j <= it; ++j) {
            launch_gmres_mgs_fold(st, n, nx, j > 0 ? d_V.p + (size_t)(j - 1) * ldv : nullptr,
                                  j > 0 ? k.gm_h(j - 1, it) : nullptr, d_V.p + (size_t)j * ldv, pin, pout, s, k.lead,
                                  ++k.lead_tag);
            std::swap(pin, pout);
        }
        launch_gmres_mgs_fold(st, n, nx, v_it, k.gm_h(it, it), nullptr, pin, pout, s, k.lead, ++k.lead_tag);
        fg.part[0] = pout;
        fg.check_after = 1;
        OGL_TRY(finalize(FIN_GMRES_COL, fg));  // ||nx||, Givens, residual-norm recurrence, the next turn's check
        fg.check_after = 0;
        fg.part[0] = d_part0.p;
    } else {
        for (int j = 0; j <= it; ++j) {
            launch_gmres_mgs(st, n, nx, j > 0 ? d_V.p + (size_t)(j - 1) * ldv : nullptr,
                             j > 0 ? k.gm_h(j - 1, it) : nullptr, d_V.p + (size_t)j * ldv,
                             d_part0.p, s);
            fg.k = j;
            OGL_TRY(finalize(FIN_GMRES_H, fg));
        }
        launch_gmres_mgs(st, n, nx, v_it, k.gm_h(it, it), nullptr, d_part0.p, s);
        fg.check_after = 1;
        OGL_TRY(finalize(FIN_GMRES_COL, fg));  // ||nx||, Givens, residual-norm recurrence, the next turn's check
        fg.check_after = 0;
    }
    if (!k.gmres_scale_late()) launch_gmres_scale(st, n, nx, nx, k.beta_ptr, s);
    return OGL_OK;
}

// The Arnoldi step of turn_gmres on a basis stored in fp32 (property basisPrecision single, orthoMethod cgs | cgs2): the
// head stores V_it = fl32((r | the last turn's nx) / its norm) and hands wide(V_it) on; nx stays fp64 in its own buffer.
int ogl_solver::turn_gmres_f32_basis(KrylovRun &k, int it, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    const int64_t ld = k.ldvf;
    DevScalars *s = k.s;
    FinArgs &fg = k.fg;
    double *nx = k.nx_buf;
    float *v_it = d_Vf.p + (size_t)it * ld;
    const double *w = d_w.p;
    if (k.generic) {  // (z is free during a turn: the x update alone uses it)
        launch_gmres_head_f32(st, n, v_it, it == 0 ? d_r.p : nx, k.beta_ptr, nullptr, d_z.p, s);
        apply_preconditioner(d_z.p, d_w.p, s);
    } else {
        launch_gmres_head_f32(st, n, v_it, it == 0 ? d_r.p : nx, k.beta_ptr, precond, d_w.p, s);
    }
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, w, nullptr, nx, SpmvDots{}, s));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    fg.turn = it;
    fg.n_sums = 1;
    const int nv = it + 1;
    launch_gmres_multidot(st, n, nx, d_Vf.p, ld, nv, d_gs_part.p, s);
    launch_gmres_fin_h(st, n, s, d_gs_part.p, nv, d_gs_h.p, k.gm_h(0, it), false);
    if (k.ortho == 2) {
        launch_gmres_block_update(st, n, nx, d_Vf.p, ld, nv, d_gs_h.p, nullptr, d_gs_part.p, s);
        launch_gmres_fin_h(st, n, s, d_gs_part.p, nv, d_gs_h.p, k.gm_h(0, it), true);
    }
    launch_gmres_block_update(st, n, nx, d_Vf.p, ld, nv, d_gs_h.p, d_part0.p, nullptr, s);
    fg.check_after = 1;
    OGL_TRY(finalize(FIN_GMRES_COL, fg));  // ||nx||, Givens, residual-norm recurrence, the next turn's check
    fg.check_after = 0;
    return OGL_OK;
}

// Property orthoTimedLaunches > 0 (measurements only; after a solve on orthoMethod cgs | cgs2, on its buffers): that many
// launches of every kernel of the block form at columns it = 0, 15 and 29 (as far as krylovDim goes), timed with HIP
// events -> orthoMultidotUs_<it>, orthoFinHUs_<it>, orthoUpdateUs_<it> (with the w . w partials), orthoUpdateDotsUs_<it>
// (with cgs2's second-round partials).  The coefficients are zeroed first: the update leaves the basis as it is.
int ogl_solver::time_ortho_kernels(KrylovRun &k)
{
    const int timed = (int)knob<Knob::orthoTimedLaunches>();
    if (timed <= 0 || !k.ortho) return OGL_OK;
    hipStream_t st = k.st;
    EventPair ev;
    OGL_HIP_CHECK(ev_create(&ev[0]));
    OGL_HIP_CHECK(ev_create(&ev[1]));
    OGL_HIP_CHECK(hipMemsetAsync(d_gs_h.p, 0, d_gs_h.n * sizeof(double), st));
    for (const int it : {0, 15, 29}) {
        if (it >= k.m) break;
        const int nv = it + 1;
        double *w = k.basis_single ? k.nx_buf : d_V.p + (size_t)nv * k.ldv, *col = k.gm_h(0, it);
        const char *names[4] = {"orthoMultidotUs_", "orthoFinHUs_", "orthoUpdateUs_", "orthoUpdateDotsUs_"};
        for (int which = 0; which < 4; ++which) {
            for (int i = -1; i < timed; ++i) {  // (i == -1: warm-up)
                if (i == 0) OGL_HIP_CHECK(hipEventRecord(ev[0], st));
                double *const pn = which == 2 ? d_part0.p : nullptr, *const pd = which == 3 ? d_gs_part.p : nullptr;
                if (which == 1) launch_gmres_fin_h(st, k.n, nullptr, d_gs_part.p, nv, d_gs_h.p, col, false);
                if (which == 0 && k.basis_single) launch_gmres_multidot(st, k.n, w, d_Vf.p, k.ldvf, nv, d_gs_part.p, nullptr);
                if (which == 0 && !k.basis_single) launch_gmres_multidot(st, k.n, w, d_V.p, k.ldv, nv, d_gs_part.p, nullptr);
                if (which >= 2 && k.basis_single) launch_gmres_block_update(st, k.n, w, d_Vf.p, k.ldvf, nv, d_gs_h.p, pn, pd, nullptr);
                if (which >= 2 && !k.basis_single) launch_gmres_block_update(st, k.n, w, d_V.p, k.ldv, nv, d_gs_h.p, pn, pd, nullptr);
            }
            OGL_HIP_CHECK(hipEventRecord(ev[1], st));
            if (which == 1) OGL_HIP_CHECK(hipMemsetAsync(d_gs_h.p, 0, d_gs_h.n * sizeof(double), st));
            OGL_HIP_CHECK(hipEventSynchronize(ev[1]));
            float ms = 0.f;
            OGL_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            props[names[which] + std::to_string(it)] = 1e3 * (double)ms / timed;
        }
    }
    return OGL_OK;
}

// GKOCG with a materialised z = M^-1 r (block Jacobi, ISAI): step_1 | SpMV | beta | step_2 | M^-1 | check
int ogl_solver::turn_cg_generic(KrylovRun &k, int, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    DevScalars *s = k.s;
    launch_cg_step1(st, n, d_p.p, d_z.p, nullptr, s);  // p = z + (rho/prev_rho) p
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, d_p.p, nullptr, d_q.p, SpmvDots{d_p.p, d_part0.p, nullptr}, s));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    OGL_TRY(finalize(FIN_BETA, k.f1));
    launch_cg_step2(st, n, d_x.p, d_r.p, d_p.p, d_q.p, nullptr, d_part0.p, d_part1.p, s);
    apply_preconditioner(d_r.p, d_z.p, s, d_part0.p);  // z = M^-1 r and the partials of r.z
    OGL_TRY(finalize(FIN_CG_CHECK, k.chk));
    return OGL_OK;
}

// ... with the leader finalisation (single rank, more than 1,024 chunks): [check of the previous turn + pending x update +
// step_1 on the materialised z] | SpMV | [beta + step_2r] | M^-1 (z and the partials of r.z); scalars s -> s2 -> s
int ogl_solver::turn_cg_generic_led(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
    double *p_new = k.p_of_turn(enq + 1);
    launch_cg_step1x_fin(st, n, k.p_of_turn(enq), d_x.p, d_z.p, nullptr, k.s, k.s2, d_part0.p, d_part1.p, d_history.p,
                         enq == 0 ? 1 : 0, k.lead, p_new, k.ring_of_turn(enq));
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, p_new, nullptr, d_q.p, SpmvDots{p_new, d_part2.p, nullptr}, k.s2));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    launch_cg_step2r_fin(st, n, d_r.p, d_q.p, nullptr, d_part0.p, d_part1.p, k.s2, k.s, d_part2.p, nullptr, k.lead);
    apply_preconditioner(d_r.p, d_z.p, k.s, d_part0.p);  // z = M^-1 r and the partials of r.z (over step_2r's r.r)
    return OGL_OK;
}

// small single-rank GKOCG on half storage, 2 launches: [check of the previous turn + pending x update + step_1 + SpMV] |
// beta + step_2r
int ogl_solver::turn_cg_two_launch(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    launch_cg_turn_sym(st, sym(), k.p_of_turn(enq), k.p_of_turn(enq + 1), d_x.p, k.z_kept ? k.z_kept : d_r.p,
                       d_q.p, d_part2.p, k.s, k.s2, d_part0.p, d_part1.p, d_history.p, enq == 0 ? 1 : 0, k.lead);
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    launch_cg_step2r_fin(st, k.n, d_r.p, d_q.p, precond, d_part0.p, d_part1.p, k.s2, k.s, d_part2.p, k.z_kept, k.lead);
    return OGL_OK;
}

// small single-rank GKOCG, 3 launches: check of the previous turn (or of the initial residual) + pending x update +
// step_1 | SpMV | beta + step_2r: the scalars go s -> s2 -> s
int ogl_solver::turn_cg_three_launch(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
    double *p_new = k.p_of_turn(enq + 1);
    launch_cg_step1x_fin(st, n, k.p_of_turn(enq), d_x.p, d_r.p, precond, k.s, k.s2, d_part0.p, d_part1.p, d_history.p,
                         enq == 0 ? 1 : 0, k.lead, p_new, k.ring_of_turn(enq));
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, p_new, nullptr, d_q.p, SpmvDots{p_new, d_part2.p, nullptr}, k.s2));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    launch_cg_step2r_fin(st, n, d_r.p, d_q.p, precond, d_part0.p, d_part1.p, k.s2, k.s, d_part2.p, nullptr, k.lead);
    return OGL_OK;
}

// The held-z turn, 2 launches: SpMV | [beta + step_2r + check + pending x update + step_1 of the NEXT turn] in one resident
// kernel that keeps z = r / d on chip (k_cg_step2r1x); the first head is the stand-alone one.  The scalars: s -> s2 by the
// first head, s2 in place from then on.
int ogl_solver::turn_cg_held_z(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    double *p_new = k.p_of_turn(enq + 1);
    if (enq == 0) {
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
        launch_cg_step1x_fin(st, n, k.p_of_turn(0), d_x.p, d_r.p, precond, k.s, k.s2, d_part0.p, d_part1.p, d_history.p, 1,
                             k.lead, p_new, k.ring_of_turn(0));
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    }
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, p_new, nullptr, d_q.p, SpmvDots{p_new, d_part2.p, nullptr}, k.s2));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    // (the head in here is turn enq + 1's: it reads the p the SpMV above has used and writes the next one)
    launch_cg_step2r1x(st, n, d_r.p, d_q.p, precond, p_new, k.p_of_turn(enq + 2), d_x.p, k.s2, d_part2.p, d_history.p, k.lead,
                       k.ring_of_turn(enq + 1), k.hz);
    return OGL_OK;
}

// The held-q turn, 1 launch: the half-storage SpMV, beta, step_2r, the check, the pending x update and step_1 of the NEXT
// turn in one resident kernel that keeps q = A p and then z = r / d on chip (k_cg_turn_held_q).  A turn with an event pair
// runs the two-launch held-z turn instead, so that the pair times the real stand-alone SpMV: both shapes leave the same
// state behind (scalars in s2, launch_seq + 2, the p ring, the pending x), and a solve may mix them freely.
int ogl_solver::turn_cg_held_q(KrylovRun &k, int enq, int pe)
{
    if (pe >= 0) return turn_cg_held_z(k, enq, pe);
    hipStream_t st = k.st;
    double *p_new = k.p_of_turn(enq + 1);
    if (enq == 0) {
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
        launch_cg_step1x_fin(st, k.n, k.p_of_turn(0), d_x.p, d_r.p, precond, k.s, k.s2, d_part0.p, d_part1.p, d_history.p, 1,
                             k.lead, p_new, k.ring_of_turn(0));
        OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    }
    launch_cg_turn_held_q(st, sym(), d_r.p, precond, p_new, k.p_of_turn(enq + 2), d_x.p, k.s2, d_history.p, k.lead,
                          k.ring_of_turn(enq + 1), k.hz, k.hq);
    if (k.hq.static_slots < HQ_STATIC) k.hq.parity ^= 1;  // (the next LAUNCH draws from the set this one has zeroed)
    return OGL_OK;
}

// Whether this solve runs the held-z turn: the leader turn of three launches (scalar Jacobi or none, one rank, p in place
// or two p buffers), by default where it streams (property heldZ), within what the resident grid holds on chip
// (heldZMaxChunks can only lower that) and only after a census launch has seen the whole grid on the chip at once.
int ogl_solver::plan_held_z(KrylovRun &k)
{
    k.hz = HeldZ{};
    k.hq = HeldQ{};
    props["heldQInUse"] = 0.0;
    props["heldQStaticSlotsInUse"] = 0.0;
    props["heldQSlotsPerGroup"] = 0.0;
    props["heldZInUse"] = 0.0;
    props["heldZGridInUse"] = 0.0;  // (the workgroups the turn launches: whether heldZGrid was honoured or clipped by the device)
    if (!(k.lead.box != nullptr && k.fused && !k.fused2 && !k.generic && !k.multi && (k.ring.k == 0 || k.ring.k == 2)))
        return OGL_OK;
    bool streams = false;
    switch (spmv_layout) {
    case SpmvLayout::Ell: streams = ell().stream; break;
    case SpmvLayout::Sell: streams = sell().stream; break;
    case SpmvLayout::Sym: streams = sym().stream; break;
    case SpmvLayout::Symx: streams = symx().stream; break;
    default: streams = csr().stream; break;
    }
    if (knob<Knob::heldZ>(streams ? 1.0 : 0.0) == 0.0 || held_z_census < 0) return OGL_OK;
    int per_wg = 0;
    int grid = held_z_grid(&per_wg);
    grid = std::min(grid, (int)knob<Knob::heldZGrid>((double)grid));  // (only ever fewer workgroups: tests reach LDS-held chunks with it)
    if (grid < 2 * 16) return OGL_OK;  // (the 2 x 16 leaders of the sums)
    const double cap = std::min((double)grid * per_wg, knob<Knob::heldZMaxChunks>((double)grid * per_wg));
    if ((double)k.nc > cap) return OGL_OK;
    // ... and the held-q turn on top of it: half storage, by default where that layout streams (property heldQ), and
    // only where the POSITIONS of its launch order -- the band order has holes, the default map is padded -- fit the slots.
    // Position w + i G lands on the XCD the stand-alone SpMV runs it on only where the grid is a multiple of the 8 XCDs:
    // any other grid (a device with such a CU count, heldZGrid) computes the same bits slower, and is on only by request.
    bool held_q = false;
    int n_pos = 0;
    if (spmv_layout == SpmvLayout::Sym) {
        n_pos = held_q_positions(sym());
        held_q = knob<Knob::heldQ>(sym().stream && grid % 8 == 0 ? 1.0 : 0.0) != 0.0 && (double)n_pos <= (double)grid * per_wg;
    }
    hipStream_t st = k.st;
    const size_t words = (held_q ? 6 : 4) * (size_t)k.nc;  // (both turn kernels of a mixed solve use the one box: the tags tell)
    if (!held_z_box || held_z_words < words) {
        ledger::dev_free(held_z_box);
        held_z_box = nullptr;
        void *b = nullptr;
        OGL_HIP_CHECK(ledger::dev_malloc(&b, words * sizeof(unsigned long long), /*fine_grained=*/true));
        held_z_box = static_cast<unsigned long long *>(b);
        held_z_words = words;
    }
    // (tags restart with every solve: no word of an earlier solve may survive)
    OGL_HIP_CHECK(hipMemsetAsync(held_z_box, 0, held_z_words * sizeof(unsigned long long), st));
    if (held_z_census == 0 || held_z_census_grid < grid) {
        void *c = nullptr;
        OGL_HIP_CHECK(ledger::dev_malloc(&c, 2 * sizeof(int)));
        int timed_out = 1;
        // (a census that cannot see everybody within a second has its answer)
        const int rc = launch_resident_census(st, grid, static_cast<unsigned *>(c), static_cast<int *>(c) + 1,
                                              (long long)(knob<Knob::heldZCensusS>() * 1e8));
        hipError_t e = rc == 0 ? hipMemcpyAsync(&timed_out, static_cast<int *>(c) + 1, sizeof(int), hipMemcpyDeviceToHost, st)
                               : hipErrorUnknown;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        ledger::dev_free(c);
        if (e != hipSuccess) return fail(OGL_ERR_HIP, "census of the held-z grid failed: %s", hipGetErrorString(e));
        held_z_census = timed_out ? -1 : 1;
        held_z_census_grid = grid;
        if (timed_out) return OGL_OK;
    }
    k.hz.tagged = held_z_box;
    k.hz.grid = grid;
    // heldZEarlyX 0 switches early x off; heldZEarlySlots: for how many of a workgroup's slots it runs.  4 by default: the
    // wait it covers is 6 us, a slot of it takes 2 us, and every slot more is 1/20 of p read twice.  Measured
    // (profiles/r11_resident_waits.txt, section 3): 0 and 4 slots run level, all 20 are slower by 2 %.
    const int early_slots = std::max(0, std::min(per_wg, (int)knob<Knob::heldZEarlySlots>()));
    k.hz.early_slots = knob<Knob::heldZEarlyX>() != 0.0 ? early_slots : 0;
    props["heldZInUse"] = 1.0;
    props["heldZGridInUse"] = (double)grid;
    if (held_q) {
        k.hq.on = 1;
        k.hq.n_pos = n_pos;
        k.hq.static_slots = HQ_STATIC;
        k.hq.drawers = grid;
        props["heldQInUse"] = 1.0;
        // Phase S draws the positions behind the first heldQStaticSlots slots from eight queues (k_cg_turn_held_q).
        // heldQIdleGroups m (a test's knob: only with no static slot, m a multiple of 8): the last m workgroups own
        // nothing, so the others fill the slots past HQ_STATIC.  The draw is complete only where, queue by queue, the
        // drawing workgroups' free slots hold the queue; anything else runs the static map.
        const int slots = HQ_R + HZ_L;
        const int S = std::max(0, std::min(HQ_STATIC, (int)knob<Knob::heldQStaticSlots>()));
        const int idle = (int)knob<Knob::heldQIdleGroups>();
        const int drawers = (S == 0 && idle > 0 && idle % N_XCD == 0 && idle < grid) ? grid - idle : grid;
        bool fits = (long long)S * grid < n_pos;  // (else there is nothing to draw)
        for (int q = 0; fits && q < N_XCD; ++q) {
            auto members = [q](long long lo, long long hi) {  // numbers in [lo, hi) that are q modulo 8
                auto below = [q](long long v) { return v <= q ? 0 : (v - q + N_XCD - 1) / N_XCD; };
                return hi > lo ? below(hi) - below(lo) : 0;
            };
            fits = members(0, drawers) * (slots - S) >= members((long long)S * grid, n_pos);
        }
        if (fits) {
            if (!held_q_heads) {
                void *h = nullptr;
                OGL_HIP_CHECK(ledger::dev_malloc(&h, HQ_HEAD_WORDS * sizeof(unsigned)));
                held_q_heads = static_cast<unsigned *>(h);
            }
            // (both sets: the parity restarts with the solve)
            OGL_HIP_CHECK(hipMemsetAsync(held_q_heads, 0, HQ_HEAD_WORDS * sizeof(unsigned), st));
            k.hq.static_slots = S;
            k.hq.drawers = drawers;
            k.hq.heads = held_q_heads;
        }
    }
    props["heldQStaticSlotsInUse"] = (double)k.hq.static_slots;
    // (the static map runs the kernel on the held-z turn's 11 + 9 slots, the draw the one on 13 + 9)
    props["heldQSlotsPerGroup"] = !k.hq.on ? 0.0 : (double)((k.hq.static_slots < HQ_STATIC ? HQ_R : HZ_R) + HZ_L);
    return OGL_OK;
}

// GKOCG on half storage between the single-workgroup finalisers, 4 launches: [pending x update + step_1 + SpMV] | beta |
// step_2r (keeps z) | check; several ranks: the neighbours' step_2r has put z, p_new is formed at the halo columns here
int ogl_solver::turn_cg_merged(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    DevScalars *s = k.s;
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    if (k.merged_halo) {
        // (waits for the z the neighbours put one kernel -- or, before turn 0, one launch -- earlier)
        launch_cg_turn_sym_big(st, sym(), k.p_of_turn(enq), k.p_of_turn(enq + 1), d_x.p,
                               k.z_kept ? k.z_kept : d_r.p, d_q.p, d_part0.p, s,
                               halo_fused_args(cur_halo), k.p_halo_of_turn(enq), k.p_halo_of_turn(enq + 1));
    } else {
        launch_cg_turn_sym_big(st, sym(), k.p_of_turn(enq), k.p_of_turn(enq + 1), d_x.p,
                               k.z_kept ? k.z_kept : d_r.p, d_q.p, d_part0.p, s);
    }
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    OGL_TRY(finalize(FIN_BETA, k.f1));
    if (k.merged_halo) {
        const HaloPutFused put = begin_halo_put();  // z of the next turn
        launch_cg_step2r(st, n, d_r.p, d_q.p, precond, d_part0.p, d_part1.p, s, k.z_kept, &put);
    } else {
        launch_cg_step2r(st, n, d_r.p, d_q.p, precond, d_part0.p, d_part1.p, s, k.z_kept);
    }
    k.chk.turn = 1;  // this check leaves an x update pending for the next turn's kernel
    OGL_TRY(finalize(FIN_CG_CHECK, k.chk));
    return OGL_OK;
}

// GKOCG, 5 launches (the headline's turn): step_1x | SpMV | beta | step_2r | check.  x += t p is deferred into the next
// turn's step_1x (kernels_krylov.hip): p is read once (peer-put transport: the halo values of the SpMV are put by step_1x itself)
int ogl_solver::turn_cg_five_launch(KrylovRun &k, int, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    DevScalars *s = k.s;
    const HaloPutFused put = begin_halo_put();
    launch_cg_step1x(st, n, d_p.p, d_x.p, d_r.p, precond, s, &put);
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, d_p.p, nullptr, d_q.p,
                      SpmvDots{d_p.p, d_part0.p, nullptr}, s, put.chunk_sptr != nullptr));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    OGL_TRY(finalize(FIN_BETA, k.f1));
    launch_cg_step2r(st, n, d_r.p, d_q.p, precond, d_part0.p, d_part1.p, s);
    k.chk.turn = 1;  // this check leaves an x update pending for the next step_1x
    OGL_TRY(finalize(FIN_CG_CHECK, k.chk));
    return OGL_OK;
}

// small single-rank GKOBiCGStab, 5 launches + the preconditioner's own: [check + step_1] | M^-1 | SpMV | [alpha + step_2] |
// M^-1 | SpMV | [mid-turn check + omega + step_3]; partials: rho, sum|r| in part0 / part1; rr.v in part2; sum|s| in
// part3; s.t, t.t in part4 / part5; the scalars alternate between the two slots (k.cur)
int ogl_solver::turn_bicg_folded(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    DevScalars **slot_s = k.slot_s;
    int &cur = k.cur;
    double *y = k.y, *z = k.z;
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[0], st));
    launch_bicg_fold1(st, n, d_p.p, d_r.p, d_v.p, precond, y, slot_s[cur], slot_s[cur ^ 1], d_part0.p,
                      d_part1.p, d_history.p, k.lead);
    cur ^= 1;
    if (enq == 0) OGL_HIP_CHECK(hipEventRecord(k.ev_chk[1], st));
    if (k.generic) apply_preconditioner(d_p.p, y, slot_s[cur]);
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, y, nullptr, d_v.p, SpmvDots{d_rr.p, d_part2.p, nullptr}, slot_s[cur]));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    launch_bicg_fold2(st, n, d_r.p, d_v.p, d_s.p, precond, z, d_part3.p, slot_s[cur], slot_s[cur ^ 1],
                      d_part2.p, k.lead);
    cur ^= 1;
    if (k.generic) apply_preconditioner(d_s.p, z, slot_s[cur]);
    OGL_TRY(dist_spmv(SPMV_PLAIN, z, nullptr, d_t.p, SpmvDots{d_s.p, d_part4.p, d_part5.p}, slot_s[cur]));
    launch_bicg_fold3(st, n, d_x.p, d_r.p, d_s.p, d_t.p, y, z, d_rr.p, d_part0.p, d_part1.p, slot_s[cur],
                      slot_s[cur ^ 1], d_part4.p, d_part5.p, d_part3.p, d_history.p, enq, k.lead);
    cur ^= 1;
    return OGL_OK;
}

// GKOBiCGStab, 8 launches + the preconditioner's own (9 with several ranks: the mid-turn check keeps its own finaliser)
int ogl_solver::turn_bicg(KrylovRun &k, int enq, int pe)
{
    hipStream_t st = k.st;
    const int n = k.n;
    DevScalars *s = k.s;
    double *y = k.y, *z = k.z;
    FinArgs &f1 = k.f1, &f2 = k.f2;
    launch_bicg_step1(st, n, d_p.p, d_r.p, d_v.p, precond, y, s);
    if (k.generic) apply_preconditioner(d_p.p, y, s);
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe], st));
    OGL_TRY(dist_spmv(SPMV_PLAIN, y, nullptr, d_v.p,
                      SpmvDots{d_rr.p, d_part0.p, nullptr}, s));
    if (pe >= 0) OGL_HIP_CHECK(hipEventRecord(prof_ev[2 * pe + 1], st));
    OGL_TRY(finalize(FIN_BICG_ALPHA, f1));
    if (!k.multi && knob<Knob::bicgMergedCheck>() != 0.0) {
        // single rank: the mid-turn check moves behind the second SpMV and shares its finaliser (8 launches
        // per turn instead of 9; when it stops the solve that SpMV ran for nothing)
        launch_bicg_step2(st, n, d_r.p, d_v.p, d_s.p, precond, z, d_part2.p, s);
        if (k.generic) apply_preconditioner(d_s.p, z, s);
        OGL_TRY(dist_spmv(SPMV_PLAIN, z, nullptr, d_t.p,
                          SpmvDots{d_s.p, d_part0.p, d_part1.p}, s));
        FinArgs f3 = f2;
        f3.part_extra = d_part2.p;
        f3.n_sums = 3;
        f3.turn = enq;
        OGL_TRY(finalize(FIN_BICG_CHECK2_OMEGA, f3));
    } else {
        launch_bicg_step2(st, n, d_r.p, d_v.p, d_s.p, precond, z, d_part0.p, s);
        if (k.generic) apply_preconditioner(d_s.p, z, s);
        f1.turn = enq;
        OGL_TRY(finalize(FIN_BICG_CHECK2, f1));
        OGL_TRY(dist_spmv(SPMV_PLAIN, z, nullptr, d_t.p,
                          SpmvDots{d_s.p, d_part0.p, d_part1.p}, s));
        OGL_TRY(finalize(FIN_BICG_OMEGA, f2));
    }
    launch_bicg_step3(st, n, d_x.p, d_r.p, d_s.p, d_t.p, y, z, d_rr.p, d_part0.p,
                      d_part1.p, s, enq);
    OGL_TRY(finalize(FIN_CG_CHECK, k.chk));
    return OGL_OK;
}

// `count` turns into the stream, each in its solver's / system's shape
int ogl_solver::krylov_enqueue(KrylovRun &k, int count)
{
    for (int i = 0; i < count; ++i, ++k.enq) {
        const int enq = k.enq;
        const bool prof = k.prof_stride && enq % k.prof_stride == 0 && enq / k.prof_stride < k.prof_cap;
        const int pe = prof ? enq / k.prof_stride : -1;  // event pair of this turn
        if (k.gmres)
            OGL_TRY(turn_gmres(k, enq, pe));
        else if (k.bicg)
            OGL_TRY(k.bicg_fold ? turn_bicg_folded(k, enq, pe) : turn_bicg(k, enq, pe));
        else if (k.generic)
            OGL_TRY(k.fused ? turn_cg_generic_led(k, enq, pe) : turn_cg_generic(k, enq, pe));
        else if (k.fused2)
            OGL_TRY(turn_cg_two_launch(k, enq, pe));
        else if (k.held_z())
            OGL_TRY(k.hq.on ? turn_cg_held_q(k, enq, pe) : turn_cg_held_z(k, enq, pe));
        else if (k.fused)
            OGL_TRY(turn_cg_three_launch(k, enq, pe));
        else if (k.merged)
            OGL_TRY(turn_cg_merged(k, enq, pe));
        else
            OGL_TRY(turn_cg_five_launch(k, enq, pe));
    }
    return OGL_OK;
}

// GKOCG: gko::solver::Cg step order ([UPSTREAM]) with the OpenFOAM criterion
// evaluated on the device.  Per turn:
//   (z = M^-1 r, rho = r.z, sum|r|)  -> check -> p = z + (rho/prev_rho) p -> q = A p, beta = p.q
//   -> x += (rho/beta) p, r -= (rho/beta) q
// The host only enqueues; it looks at the stop flag one batch late, and kernels enqueued after
// the stop are no-ops, so x, r and the counters are exactly those of the stopping turn.
int ogl_solver::krylov_loop(KrylovRun &k)
{
    hipStream_t st = k.st;
    const bool fused = k.fused;
    auto poll_record = [&](int slot) -> int {
        // (the held-z turn keeps the scalars in s2; every other folded CG turn ends with them in s)
        OGL_HIP_CHECK(hipMemcpyAsync(&h_scal[slot], k.bicg_fold ? k.slot_s[k.cur] : (k.held_z() ? k.s2 : k.s), sizeof(DevScalars),
                                     hipMemcpyDeviceToHost, st));
        OGL_HIP_CHECK(hipEventRecord(poll_ev[slot], st));
        return OGL_OK;
    };

    // The host never waits for the turn it has just enqueued: it looks at the stop flag of batch j
    // only after batch j+1 is in the queue.  Every rank sees the same flags (the norms are
    // all-reduced), hence enqueues the same number of batches and of RCCL calls.
    const int batch = k.bicg ? 8 : 16;

    // hipGraph replay of a full batch of single-rank GKOCG turns (property "hipGraph").  Nothing in the
    // captured launches depends on the turn or on the solve (criterion and flags live in the device
    // scalars); the key lists every pointer they do bake in.  For the 5-launch turn it does not pay on
    // MI355X / ROCm 7.2 (23.7 us per turn with plain stream launches against 24.2 us replayed at 262k rows,
    // 286.1 against 285.3 us at 10M rows: the gap between two dependent kernels is the device's dispatch
    // latency, not host launch cost) and stays off by default.
    const bool graphable = !k.gmres && !k.bicg && !k.generic && !k.multi && k.prof_cap == 0 &&
                           knob<Knob::hipGraph>(fused ? 1.0 : 0.0) != 0.0;
    // (on by default for the folded 2- / 3-launch turns of small systems, where the host's launch rate shows: 32^3
    //  15.1 -> 13.0 us per 3-launch turn, 64^3 17.3 -> 16.7; the 5-launch turn of larger systems measures the same either way;
    //  a batch of 16 turns leaves the two p buffers of the 2-launch turn where it found them)
    auto enqueue_turns = [&](int count) -> int {
        // (the fused-finaliser turn: its first step_1x_fin differs from the later ones -- the first batch runs direct)
        if (!graphable || count != batch || (fused && k.enq == 0)) return krylov_enqueue(k, count);
        // the key: every view a captured launcher reads, hashed field by field (launch_key.hpp), the vectors and scalar
        // slots the turn kernels take, the turn's shape, and the pattern the layouts belong to (a rebuild with the same
        // sizes usually gets the same pointers back: 32x64x32 -> 64x32x32)
        KeyHasher kh;
        kh(k.n), kh(batch), kh(cfg.matrix_format), kh(spmv_layout);
        kh(k.fused), kh(k.fused2), kh(k.merged), kh(k.ring.k), kh(k.p0), kh(k.p1), kh(k.z_kept), kh(k.s), kh(k.s2), kh(pat_id);
        for (const void *v : {(const void *)d_p.p, (const void *)d_x.p, (const void *)d_r.p, (const void *)d_q.p,
                              (const void *)precond, (const void *)d_part0.p, (const void *)d_part1.p,
                              (const void *)d_part2.p, (const void *)d_history.p, (const void *)d_z.p, (const void *)d_p2.p})
            kh(v);
        for (int i = 0; i < k.ring.k; ++i) kh((const void *)k.ring.b[i]);
        visit(kh, csr());  // (also what the generation kernels read)
        switch (spmv_layout) {  // (a captured turn reads the selected layout only)
        case SpmvLayout::Ell: visit(kh, ell()); break;
        case SpmvLayout::Sell: visit(kh, sell()); break;
        case SpmvLayout::Sym: visit(kh, sym()); break;
        case SpmvLayout::Symx: visit(kh, symx()); break;
        default: break;  // (Csr, Csr21: csr() above)
        }
        visit(kh, k.lead);
        visit(kh, k.hz);
        visit(kh, k.hq);
        visit(kh, k.basis);  // (GKOGMRES turns are not captured today; the basis a captured one would bake in is in the key)
        const uint64_t key = kh.h;
        if (!cg_graph || key != cg_graph_key) {
            if (cg_graph) {
                (void)hipGraphExecDestroy(cg_graph);
                ledger::destroyed(ledger::GRAPH_EXEC);
            }
            cg_graph = nullptr;
            OGL_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            const int before = k.enq;
            const int rc = krylov_enqueue(k, batch);
            k.enq = before;  // captured, not run
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(st, &g);
            if (rc != OGL_OK || e != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);
                return rc != OGL_OK ? rc : fail(OGL_ERR_HIP, "stream capture failed: %s", hipGetErrorString(e));
            }
            const hipError_t ei = hipGraphInstantiate(&cg_graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) {
                cg_graph = nullptr;
                return fail(OGL_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
            }
            ledger::created(ledger::GRAPH_EXEC);
            cg_graph_key = key;
            set_knob<Knob::hipGraphCaptures>(knob<Knob::hipGraphCaptures>() + 1.0);
        }
        OGL_HIP_CHECK(hipGraphLaunch(cg_graph, st));
        k.enq += batch;
        return OGL_OK;
    };
    OGL_TRY(enqueue_turns(std::min(batch, k.max_turns - k.enq)));
    OGL_TRY(poll_record(0));
    for (int j = 0;; ++j) {
        const bool more = k.enq < k.max_turns;
        if (more) {
            OGL_TRY(enqueue_turns(std::min(batch, k.max_turns - k.enq)));
            OGL_TRY(poll_record((j + 1) & 1));
        }
        OGL_HIP_CHECK(hipEventSynchronize(poll_ev[j & 1]));
        if (h_scal[j & 1].stop) break;
        if (!more && k.folded()) break;  // (the check of the last enqueued turn is still to come: krylov_finish)
        if (!more) return fail(OGL_ERR_STATE, "criterion did not stop within maxIter + frequency");
    }
    return OGL_OK;
}

// The closing check of the folded turns, the pending x update, GMRES' final solve_krylov; history, perf, the
// properties the adaptive criterion of the next solve reads.
int ogl_solver::krylov_finish(KrylovRun &k, ogl_perf *perf)
{
    hipStream_t st = k.st;
    const int n = k.n, m = k.m;
    DevScalars *s = k.s, *s2 = k.s2;
    const bool bicg = k.bicg, gmres = k.gmres, fused = k.fused, bicg_fold = k.bicg_fold;
    // the check that closes the last turn run so far (a plain copy s -> s2 when the solve has stopped); the held-z turn's
    // last kernel has run it already and left the scalars in s2
    if (fused && !k.held_z())
        launch_cg_step1x_fin(st, n, k.p_of_turn(k.enq), d_x.p, k.generic ? d_z.p : d_r.p, k.generic ? nullptr : precond, s, s2,
                             d_part0.p, d_part1.p, d_history.p, 0, k.lead, k.p_of_turn(k.enq + 1), k.ring_of_turn(k.enq));
    if (bicg_fold) {  // the check that closes the last turn run so far (a plain copy of the scalars when the solve has stopped)
        launch_bicg_fold1(st, n, d_p.p, d_r.p, d_v.p, precond, k.y, k.slot_s[k.cur], k.slot_s[k.cur ^ 1], d_part0.p,
                          d_part1.p, d_history.p, k.lead);
        k.cur ^= 1;
    }
    DevScalars *fin_s = bicg_fold ? k.slot_s[k.cur] : (fused ? s2 : s);
    if (const int32_t *word = precond_breakdown_word())  // (the preconditioner's breakdown word travels with the final scalars)
        OGL_HIP_CHECK(hipMemcpyAsync(&fin_s->factor_breakdown, word, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    OGL_HIP_CHECK(hipStreamSynchronize(st));
    OGL_HIP_CHECK(hipGetLastError());
    DevScalars fin;
    OGL_HIP_CHECK(hipMemcpy(&fin, fin_s, sizeof(fin), hipMemcpyDeviceToHost));
    OGL_TRY(check_factor_breakdown(fin.factor_breakdown));  // (IC / ILU / IRILU: a broken-down factor fails the solve)
    OGL_TRY(check_chebyshev_breakdown(fin.factor_breakdown));  // (Chebyshev: a bound that is not finite and positive)
    if (k.folded() && !fin.stop) return fail(OGL_ERR_STATE, "criterion did not stop within maxIter + frequency");
    if (fin.comm_error && !k.multi && k.lead.box)
        return fail(OGL_ERR_STATE, "leader finalisation timed out: the sums of a turn were not published within "
                    "leadTimeoutS = %g s (check %d)", knob<Knob::leadTimeoutS>(), fin.iter);
    if (fin.comm_error)
        return fail(OGL_ERR_COMM, "peer all-reduce timed out: a rank did not take part (check %d)",
                    fin.iter);
    if (fin.x_pending) {
        // the stop came with the check of the last enqueued turn: no step_1x followed to apply
        // that turn's x update
        launch_cg_step1x(st, n, k.p_of_turn(k.enq), d_x.p, d_r.p, precond, s);
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_HIP_CHECK(hipGetLastError());
    }
    if (gmres) {
        // final solve_krylov on the (partial) cycle: Arnoldi steps done since the last restart
        const int steps = fin.iter - 1;
        const int cols = steps <= 0 ? 0 : (steps - 1) % m + 1;
        OGL_TRY(gmres_update_x(k, cols, nullptr));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_HIP_CHECK(hipGetLastError());
    }
    const double t_solve = now_ms() - k.t_start;
    OGL_TRY(time_ortho_kernels(k));
    history.clear();
    if (cfg.export_res) {
        history.resize(fin.iter);
        OGL_HIP_CHECK(hipMemcpy(history.data(), d_history.p, (size_t)fin.iter * sizeof(double),
                                hipMemcpyDeviceToHost));
    }
    float chk_ms = 0.f;
    OGL_HIP_CHECK(hipEventElapsedTime(&chk_ms, k.ev_chk[0], k.ev_chk[1]));

    // where the multi-rank turns of this solve waited (DevScalars, kernels.hpp; wall_clock64 counts 10 ns)
    props["turnsEnqueued"] = (double)k.enq;  // (the host looks at the stop flag one batch late: at most two batches past the stop)
    props["haloWaits"] = (double)fin.halo_waits;
    props["haloWaitUs"] = (double)fin.halo_wait_ticks / 100.0;
    props["allreduceWaits"] = (double)fin.reduce_waits;
    props["allreduceWaitUs"] = (double)fin.reduce_wait_ticks / 100.0;
    props["peerSafeWaitInUse"] = (pat.non_local_nnz > 0 && peer_halo && peer_safe_wait()) ? 1.0 : 0.0;
    props["peerSharedDevice"] = reg->peer_shared_device ? 1.0 : 0.0;
    perf->initial_residual = fin.init_res;                  // lduLduBase.H:283
    perf->final_residual = fin.res;                         // :284
    perf->n_iterations = bicg ? fin.iter / 2 : fin.iter;    // :285, GKOCG.H:105-108, GKOBiCGStab.H:114
    perf->n_norm_evals = fin.n_evals;
    perf->norm_factor = fin.norm_factor;
    perf->t_solve_ms = t_solve;
    const int turns_done = bicg ? fin.iter / 2 : std::max(0, fin.iter - 1);
    perf->spmv_avg_ms = 0;
    perf->spmv_launches = 0;
    if (k.prof_cap) {
        double acc = 0;
        const int cnt = std::min((turns_done + k.prof_stride - 1) / k.prof_stride, k.prof_cap);
        for (int i = 0; i < cnt; ++i) {
            float ms = 0.f;
            OGL_HIP_CHECK(hipEventElapsedTime(&ms, prof_ev[2 * i], prof_ev[2 * i + 1]));
            acc += ms;
        }
        perf->spmv_launches = cnt;
        perf->spmv_avg_ms = cnt ? acc / cnt : 0.0;
    }

    // store_number_of_iterations + relative residual-evaluation cost (lduLduBase.H:286-293);
    // both are stored as labels, i.e. truncated (common.C:75-76,117-123).  The stored count is the
    // raw number of checks for every solver (GKOBiCGStab.H:98-103).
    k.is_final ? set_knob<Knob::prevSolveIters_final>(fin.iter) : set_knob<Knob::prevSolveIters>(fin.iter);
    const double time_per_iter = t_solve * 1e3 / std::max(perf->n_iterations, 1);
    const double res_norm_time = std::max(1e-3, (double)chk_ms * 1e3);
    double rel_cost = time_per_iter / res_norm_time;
    perf->t_res_norm_us = res_norm_time;
    perf->n_global_rows = k.n_global;
    if (reg->comm->multi()) {  // broadcast from rank 0 (:291-292) so every rank adapts alike
        double v = reg->comm->rank == 0 ? rel_cost : 0.0;
        OGL_HIP_CHECK(hipMemcpy(sums_ptr(s), &v, sizeof(double), hipMemcpyHostToDevice));
        OGL_TRY(reg->allreduce(sums_ptr(s), 1));
        OGL_HIP_CHECK(hipStreamSynchronize(st));
        OGL_HIP_CHECK(hipMemcpy(&rel_cost, sums_ptr(s), sizeof(double), hipMemcpyDeviceToHost));
    }
    set_knob<Knob::_prev_solve>(std::floor(rel_cost));
    return OGL_OK;
}

// solver->apply(b, x) on the resident vectors (lduLduBase.H:254-276)
int ogl_solver::apply_resident(ogl_perf *perf)
{
    if (!matrix_set) return fail(OGL_ERR_STATE, "solve before set_matrix");
    if (!x_resident || !b_resident) return fail(OGL_ERR_STATE, "rhs/solution not resident");
    OGL_HIP_CHECK(hipSetDevice(reg->device));
    ogl_perf local{};
    if (!perf) perf = &local;
    TraceRange trace("solve", field);
    bool mixed_on = false;  // (refused before anything is generated for it)
    OGL_TRY(mixed_requested(&mixed_on));
    int ortho = 0;
    OGL_TRY(ortho_requested(&ortho));
    bool basis_single = false;
    OGL_TRY(basis_requested(&basis_single));
    int proj_k = 0;
    OGL_TRY(proj_requested(&proj_k));
    // (keyword guessProjection: d_x becomes the projected guess, and from here on the solve is the one called with it)
    bool proj_cr = false;
    OGL_TRY(proj_credit_requested(proj_k, mixed_on, &proj_cr));
    bool proj_one_pass = false;
    OGL_TRY(proj_products_requested(&proj_one_pass));
    OGL_TRY(proj_pre_step(proj_k, proj_cr, proj_one_pass));
    {
        TraceRange trace_pc("init_preconditioner", field);
        OGL_TRY(init_preconditioner());
    }
    int rc = OGL_OK;
    switch (cfg.solver) {
    case OGL_SOLVER_CG:
        rc = run_cg(perf);
        break;
    case OGL_SOLVER_BICGSTAB:
        rc = run_bicgstab(perf);
        break;
    case OGL_SOLVER_GMRES:
        rc = run_krylov(perf);
        break;
    default:
        return fail(OGL_ERR_UNSUPPORTED, "solver kind %d is not built", cfg.solver);
    }
    return proj_post_step(rc, perf);
}

// lduLduBase::solve_multi_gpu_impl (lduLduBase.H:189-308)
int ogl_solver::solve(const double *source, double *psi, ogl_perf *perf)
{
    if (!matrix_set) return fail(OGL_ERR_STATE, "solve before set_matrix");
    if (!source || !psi) return fail(OGL_ERR_INVALID, "source/psi is NULL");
    OGL_HIP_CHECK(hipSetDevice(reg->device));
    hipStream_t st = reg->stream;
    ogl_perf local{};
    if (!perf) perf = &local;
    *perf = ogl_perf{};
    const double t0 = now_ms();
    {
        TraceRange trace("upload_rhs_and_guess", field);
        if (!b_resident || cfg.update_rhs) {  // :217-226
            OGL_TRY(upload_vec(d_b, source));
            b_resident = true;
        }
        if (!x_resident || cfg.update_init_guess) {  // :228-237
            OGL_TRY(upload_vec(d_x, psi));
            x_resident = true;
        }
        if (cfg.scaling != 1.0) launch_scale(st, pat.n_rows, d_b.p, cfg.scaling);  // :242-252
        OGL_HIP_CHECK(hipStreamSynchronize(st));
    }
    perf->t_upload_ms = now_ms() - t0;
    perf->t_update_matrix_ms = t_update_matrix_ms;
    OGL_TRY(apply_resident(perf));
    const double t1 = now_ms();
    {
        TraceRange trace("copy_back", field);
        OGL_TRY(download_rows(psi, d_x.p));  // :278-279
    }
    perf->t_copy_back_ms = now_ms() - t1;
    return OGL_OK;
}

// `repeats` in-loop SpMVs (q = A b, fused dot) timed with HIP events on the solver's stream
int ogl_solver::time_spmv(int repeats, double *avg_ms)
{
    if (!matrix_set) return fail(OGL_ERR_STATE, "time_spmv before set_matrix");
    OGL_HIP_CHECK(hipSetDevice(reg->device));
    hipStream_t st = reg->stream;
    EventPair ev;
    OGL_HIP_CHECK(ev_create(&ev[0]));
    OGL_HIP_CHECK(ev_create(&ev[1]));
    hipEvent_t e0 = ev[0], e1 = ev[1];
    OGL_TRY(dist_spmv(SPMV_PLAIN, d_b.p, nullptr, d_q.p, SpmvDots{d_b.p, d_part0.p, nullptr}, nullptr));  // warm-up
    OGL_HIP_CHECK(hipEventRecord(e0, st));
    for (int i = 0; i < repeats; ++i) {
        // alternate the input so consecutive launches do not read what the last one wrote
        const double *x = (i & 1) ? d_r.p : d_b.p;
        OGL_TRY(dist_spmv(SPMV_PLAIN, x, nullptr, d_q.p, SpmvDots{x, d_part0.p, nullptr}, nullptr));
    }
    OGL_HIP_CHECK(hipEventRecord(e1, st));
    OGL_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OGL_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = repeats > 0 ? (double)ms / repeats : 0.0;
    return OGL_OK;
}
