// properties.hpp -- every property a solver reads as an INPUT, declared once: name, default, domain, one line of text.
// ogl_solver::props (a string -> double map, the reference's per-field store, common/common.C:75-146) keeps the values;
// the library reads them only through ogl_solver::knob<Knob::name>(), so a misspelt name does not compile and a default
// stands in one place.  Reports (`...InUse`, sizes, timings) are plain writes to the map and are not listed here.
//
// A new keyword: one line in OGL_KNOBS, a row in INTEGRATION.md section 6 (tests/test_property_table.py compares the two).
#pragma once

#include <cstdint>
#include <limits>

#include "kernels.hpp"

namespace ogl {

// where a knob's default comes from
enum class KnobKind : int32_t {
    Fixed = 0,     // the table's number
    Computed = 1,  // the call site's: it depends on the environment or on the run (the entry says on what)
    State = 2,     // the reference's per-field store and its kin: the library reads AND writes them
};

struct KnobDefault {
    KnobKind kind;
    double value;      // Fixed, State (what a read finds before the first write); NaN for Computed
    const char *what;  // Computed: what the call site supplies
};
constexpr KnobDefault fixed(double v) { return {KnobKind::Fixed, v, nullptr}; }
constexpr KnobDefault computed(const char *what) { return {KnobKind::Computed, std::numeric_limits<double>::quiet_NaN(), what}; }
constexpr KnobDefault state(double v) { return {KnobKind::State, v, nullptr}; }

// what ogl_solver::check_knob accepts; only the properties that were validated before the table have one
struct KnobDomain {
    enum Type { None, Flag, Whole, Choice, Open } type;
    double lo, hi;      // Whole: integral in [lo, hi]; Open: lo < v < hi; Choice: 0 .. hi
    const char *words;  // Choice: the words of 0, 1, ... separated by '|'
};
constexpr KnobDomain none() { return {KnobDomain::None, 0.0, 0.0, nullptr}; }
constexpr KnobDomain flag() { return {KnobDomain::Flag, 0.0, 1.0, nullptr}; }
constexpr KnobDomain whole(double lo, double hi) { return {KnobDomain::Whole, lo, hi, nullptr}; }
constexpr KnobDomain open(double lo, double hi) { return {KnobDomain::Open, lo, hi, nullptr}; }
constexpr KnobDomain choice(const char *words)
{
    int n = 0;
    for (const char *p = words; *p; ++p) n += *p == '|';
    return {KnobDomain::Choice, 0.0, (double)n, words};
}

constexpr bool WRITTEN_BACK = true;  // the library overwrites the caller's value with the one in effect

// X(name, default, domain, written back, text)
#define OGL_KNOBS(X) \
    /* ---- set-up of the device matrix ---- */ \
    X(deviceSetup, fixed(1.0), none(), WRITTEN_BACK, \
      "0: build the pattern with the host algorithm (the checked fallback)") \
    X(renumberCurve, fixed(1.0), none(), false, "with cell centres: the Hilbert-curve candidate competes with RCM (0: RCM only)") \
    X(curveOnDevice, fixed(1.0), none(), false, "the curve's keys, sort and far-entry count run on the device (0: host code)") \
    X(symmetricHalfWhole_enable, fixed(1.0), none(), false, "experiment switch: the whole-matrix half-storage layout") \
    X(symmetricHalfPerChunk_enable, fixed(1.0), none(), false, "experiment switch: the per-chunk half-storage layout") \
    X(spmvForceLayout, fixed(-1.0), none(), false, \
      "0 / 1 / 2: CSR-stream / compressed / packed columns whatever the one-off timing says (-1: the timing decides)") \
    X(spmvBandRows, fixed(-1.0), none(), false, \
      "band-aware workgroup order of the compressed / CSR-stream kernels: the band in rows, 0 off, -1 the pattern's own") \
    X(spmvLdsRounds, fixed(1.0), none(), false, "CSR-stream kernel: 2 = its products go through LDS in two rounds") \
    X(streamAboveBytes, computed("OGL_STREAM_ABOVE_BYTES, else 288e6"), none(), false, \
      "a working set above this many bytes runs the STREAM instantiations of the SpMV kernels") \
    X(streamTurnSet, fixed(1.0), none(), false, \
      "the STREAM decision counts what a turn touches besides the system matrix (0: the matrix alone)") \
    X(xcdGroup, computed("OGL_XCD_GROUP, else what the pattern's set-up chose"), none(), false, \
      "consecutive chunks per XCD in the default workgroup -> chunk map (negative: the pattern's own choice)") \
    X(spmvStream, state(0.0), none(), false, \
      "written by the layout choice (1: the in-loop SpMV streams), read back by the ISAI applies for W and W^T") \
    /* ---- the Krylov turn ---- */ \
    X(fusedFinalizers, fixed(1.0), none(), false, "GKOCG on at most fusedFinMaxChunks chunks: finalisers folded into the step kernels") \
    X(fusedFinMaxChunks, fixed((double)FUSED_FIN_MAX_CHUNKS), none(), false, \
      "chunks of 512 rows up to which the folded finalisers run (can only lower the built-in bound)") \
    X(fusedTurn, fixed(1.0), none(), false, "small systems on half storage: step_1x merged into the SpMV kernel") \
    X(fusedTurnBig, computed("1 while the in-loop half storage does not stream, else 0"), none(), false, \
      "the same merge for systems past the folded finalisers") \
    X(fusedTurnMulti, fixed(1.0), none(), false, "several ranks on half storage with the peer mesh: step_1x inside the SpMV kernel") \
    X(haloFused, fixed(1.0), none(), false, "several ranks: halo puts inside k_cg_step1x, the non-local part inside the local SpMV") \
    X(peerSafeWait, computed("1 when peer_connect found two ranks on one device, else 0"), none(), false, \
      "peer mesh: one workgroup per rank waits for the neighbours' puts instead of every boundary workgroup") \
    X(leadFinalizers, fixed(1.0), none(), false, "one rank, large systems: the finalisers run inside the kernels that consume their scalars") \
    X(leadEarlyLoads, fixed(1.0), none(), false, "leader turn: row loads before (1) or after (0) the wait for the leaders") \
    X(leadTimeoutS, fixed(10.0), none(), false, "seconds a workgroup waits for the leaders before it fails the solve") \
    X(gmresLead, fixed(0.0), none(), false, "leader finalisation for GKOGMRES' Gram-Schmidt links (bit-equal, no faster)") \
    X(bicgFold, fixed(1.0), none(), false, "GKOBiCGStab, one rank: finalisers folded into the step kernels") \
    X(gmresFold, fixed(1.0), none(), false, "GKOGMRES, one rank, orthoMethod mgs: a link's finaliser folded into the next link") \
    X(bicgMergedCheck, fixed(1.0), none(), false, \
      "GKOBiCGStab, one rank: the mid-turn check shares the second SpMV's finaliser (0: a launch of its own)") \
    X(deferX, fixed(2.0), none(), false, "leader turn of three launches: p buffers used in turn, 2 | 4 | 8; below 2: x every turn") \
    X(deferX2, fixed(1.0), none(), false, "0: the deferred x update off whatever deferX says") \
    X(heldZ, computed("1 where the in-loop SpMV layout streams, else 0"), none(), false, \
      "the held-z turn: step_2r and the next turn's head in one resident kernel") \
    X(heldZGrid, computed("the workgroups the device holds at once"), none(), false, \
      "can only lower the held-z turn's number of resident workgroups (tests)") \
    X(heldZMaxChunks, computed("the chunks that grid holds"), none(), false, \
      "can only lower the held-z turn's capacity in chunks (tests)") \
    X(heldZCensusS, fixed(1.0), none(), false, "bound, in seconds, of the census launch that checks the held-z grid is resident at once") \
    X(heldZEarlyX, fixed(1.0), none(), false, "resident turn: x of a workgroup's first heldZEarlySlots slots updated before the sums arrive") \
    X(heldZEarlySlots, fixed(4.0), none(), false, "how many of a workgroup's slots that is (clipped to what it has)") \
    X(heldQ, computed("1 on streaming half storage with a grid that is a multiple of 8, else 0"), none(), false, \
      "the held-q turn: the half-storage SpMV joins the resident turn") \
    X(heldQStaticSlots, fixed((double)HQ_STATIC_DEFAULT), none(), false, \
      "held-q turn: a workgroup's first S slots hold positions of the static map, the others are drawn per XCD") \
    X(heldQIdleGroups, fixed(0.0), none(), false, "tests: with heldQStaticSlots 0 the last m workgroups own nothing") \
    X(hipGraph, computed("1 for the folded and leader turns, else 0"), none(), false, \
      "replay full batches of GKOCG turns as a hipGraph") \
    X(hipGraphCaptures, state(0.0), none(), false, "batches captured so far: the library counts, a caller may reset") \
    /* ---- the adaptive check frequency: the reference's per-field store ---- */ \
    X(prevSolveIters, state(1.0), none(), false, "iterations of the field's last solve with relTol != 0") \
    X(prevSolveIters_final, state(1.0), none(), false, "iterations of the field's last solve with relTol 0") \
    X(_prev_solve, state(0.0), none(), false, "cost of the last solve per iteration, in residual-norm evaluations") \
    X(preconditionerCaching, state(0.0), none(), false, "solves the stored preconditioner still serves before it is generated again") \
    /* ---- GKOGMRES ---- */ \
    X(orthoMethod, fixed(0.0), choice("mgs|cgs|cgs2"), false, "GKOGMRES: how the new Krylov vector is orthogonalised") \
    X(basisPrecision, fixed(0.0), choice("double|single"), false, "GKOGMRES: how the Krylov basis is stored (single needs cgs | cgs2)") \
    X(orthoTimedLaunches, fixed(0.0), none(), false, "measurements only: > 0 times that many launches of each orthogonalisation kernel") \
    /* ---- mixed precision ---- */ \
    X(mixedPrecision, fixed(0.0), none(), false, "GKOCG: fp32 inner CG under fp64 iterative refinement") \
    X(innerRelTol, fixed(1e-4), open(0.0, 1.0), false, "mixedPrecision: reduction an inner solve aims for") \
    X(innerMaxIter, fixed(1000.0), none(), false, "mixedPrecision: turns an inner solve may take (at least 1)") \
    X(mixedTimedSpmvs, fixed(0.0), none(), false, "measurements only: > 0 times that many fp32 products after the solve (mixedSpmvUs)") \
    /* ---- the initial guess from the last solutions ---- */ \
    X(guessProjection, fixed(0.0), whole(0, PROJ_MAX), false, "stored steps of the last solves the guess is projected on (0: off)") \
    X(guessProjectionCredit, fixed(0.0), flag(), false, "1: the criterion's initial residual is counted from the caller's guess") \
    X(guessProjectionProducts, fixed(0.0), choice("separate|onePass"), false, "A D by one launch per column or in one matrix pass") \
    X(guessProjectionReset, state(0.0), none(), false, "a write of 1 empties the field's ring at the next solve, which sets it back to 0") \
    X(guessProjectionTimed, fixed(0.0), none(), false, "measurements only: 1 = HIP events around the parts of the pre-step") \
    /* ---- preconditioners ---- */ \
    X(precondCallerNumbering, fixed(1.0), none(), false, \
      "with renumber: blocks / ISAI's triangle formed on the mesh's numbering (0: on the backend's)") \
    X(precondTimedApplies, fixed(0.0), none(), false, "measurements only: > 0 times the generation and that many applies") \
    X(jacobiFromSource, fixed(1.0), none(), false, "scalar Jacobi: 1 / d from the staged coefficient source (0: through the CSR values)") \
    X(bjGroupLanes, fixed(1.0), none(), false, "block Jacobi generated with 4 | 8 lanes per block (0: a thread per block)") \
    X(bjStagedApply, fixed(1.0), none(), false, "block Jacobi through the permutation: staged apply (0: block rows stored by device row)") \
    X(bjFusedPerm, fixed(1.0), none(), false, "the staged apply in one launch (0: three launches with two staging vectors)") \
    X(bjPermXcdGroup, fixed(0.0), none(), false, "staged apply: consecutive 512-position ranges one XCD takes (0: chosen from the size)") \
    X(isaiGroupLanes, fixed(1.0), none(), false, "ISAI generated with 4 | 8 lanes per row (0: a thread per row)") \
    X(isaiSortRows, fixed(1.0), none(), false, "ISAI: W / W^T stored longest row first per window where that earns the compressed layout") \
    X(isaiScratchBytes, fixed(2147483648.0), none(), false, "scratch shared by the dense systems of ISAI rows wider than 64 entries") \
    X(isaiKeepScratch, fixed(0.0), none(), false, "1: that scratch stays allocated after the generation") \
    X(triangularSolves, fixed(0.0), choice("exact|isai"), false, "IC / ILU: the triangular solves level by level or as two SpMVs") \
    X(factorSweeps, fixed(0.0), whole(0, 10), false, "IC / ILU / IRILU: 0 the level-scheduled factorisation, else that many fixed-point sweeps") \
    X(iluThinRows, fixed(256.0), none(), false, "IC / ILU: a run of levels of at most this many rows each is one launch") \
    /* ---- preconditioner Multigrid ---- */ \
    X(maxLevels, fixed(9.0), none(), false, "Multigrid: levels below the finest at most (negative: refused)") \
    X(minCoarseRows, fixed(10.0), none(), false, "Multigrid: coarsening stops at a level of at most this many rows") \
    X(coarseSolverIters, fixed(4.0), none(), false, "Multigrid: CG iterations on the coarsest level (negative: refused)") \
    X(cycle, fixed(0.0), none(), false, "Multigrid: 0 v | 1 w | 2 f; only v is built") \
    X(zeroGuess, fixed(1.0), none(), false, "Multigrid: the cycle starts from zero; only 1 is built") \
    X(aggregation, fixed(0.0), choice("pgm|hashed"), false, "Multigrid: how ties between neighbours are broken") \
    X(aggregatePasses, fixed(1.0), whole(1, MG_MAX_PASSES), false, "Multigrid: pairwise coarsenings per kept level") \
    X(aggregateCaching, fixed(0.0), whole(0, 1000000), false, "Multigrid: solves whose coarse values are refreshed on kept aggregates") \
    X(coarseVisits, fixed(1.0), whole(1, MG_MAX_COARSE_VISITS), WRITTEN_BACK, "Multigrid: visits of a coarse level per visit of its parent") \
    X(cyclePrecision, fixed(0.0), choice("double|single"), false, "Multigrid: operand type of the cycle") \
    X(smootherSweeps, fixed(2.0), whole(1, MG_MAX_SWEEPS), WRITTEN_BACK, "Multigrid: sweeps before and after the coarse correction") \
    X(correctionScale, fixed(1.0), open(0.0, 2.0), WRITTEN_BACK, "Multigrid: factor on the coarse correction") \
    X(mgTailRows, fixed((double)MG_TAIL_DEFAULT_ROWS), none(), WRITTEN_BACK, \
      "Multigrid: levels of at most this many rows run inside one tail kernel (clipped to what it holds)") \
    X(mgKeepStream, fixed(0.0), none(), false, "measurements only: 1 = the kept aggregate maps loaded past the caches")

enum class Knob : int32_t {
#define OGL_KNOB_ID(name, dflt, domain, written_back, text) name,
    OGL_KNOBS(OGL_KNOB_ID)
#undef OGL_KNOB_ID
};

struct KnobEntry {
    const char *name;
    KnobDefault dflt;
    KnobDomain domain;
    bool written_back;
    const char *text;
};

constexpr KnobEntry KNOBS[] = {
#define OGL_KNOB_ENTRY(name, dflt, domain, written_back, text) {#name, dflt, domain, written_back, text},
    OGL_KNOBS(OGL_KNOB_ENTRY)
#undef OGL_KNOB_ENTRY
};
constexpr int32_t N_KNOBS = (int32_t)(sizeof(KNOBS) / sizeof(KNOBS[0]));

constexpr const KnobEntry &knob_entry(Knob k) { return KNOBS[(int32_t)k]; }

// The inputs of preconditioner Chebyshev: entries of the same type, read
// and range-checked through the same code (ogl_solver::keyword<>, check_entry), in a list of their own.  OGL_KNOBS above is
// what ogl_host_property hands out, and tests/test_property_table.py pins it entry for entry to the call sites'
// defaults it was transcribed from; this list is not part of that record.
#define OGL_CHEB_KEYWORDS(X) \
    X(chebyshevDegree, fixed(4.0), whole(1, CHEB_MAX_DEGREE), false, "Chebyshev: degree of the polynomial, products per apply") \
    X(chebyshevEigRatio, fixed(30.0), open(1.0, 1e6), false, "Chebyshev: lambda_max / lambda_min of the interval the polynomial is built for") \
    X(chebyshevLambdaMax, fixed(0.0), none(), false, "Chebyshev: > 0 replaces the Gershgorin bound of D^-1 A (0: computed; negative or not finite: refused)") \
    X(chebyshevFused, fixed(1.0), none(), false, "Chebyshev on the whole-matrix half storage: product and recurrence in one kernel (0: two launches per step)")

enum class ChebKeyword : int32_t {
#define OGL_KNOB_ID(name, dflt, domain, written_back, text) name,
    OGL_CHEB_KEYWORDS(OGL_KNOB_ID)
#undef OGL_KNOB_ID
};
constexpr KnobEntry CHEB_KEYWORDS[] = {
#define OGL_KNOB_ENTRY(name, dflt, domain, written_back, text) {#name, dflt, domain, written_back, text},
    OGL_CHEB_KEYWORDS(OGL_KNOB_ENTRY)
#undef OGL_KNOB_ENTRY
};
constexpr const KnobEntry &knob_entry(ChebKeyword k) { return CHEB_KEYWORDS[(int32_t)k]; }

}  // namespace ogl
