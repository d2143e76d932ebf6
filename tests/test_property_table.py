"""The table of input properties (ogl_amd/csrc/properties.hpp) through ogl_host_property: its defaults are the ones every
call site carried before the table, its names are the keys INTEGRATION.md section 6 lists, and no read by string is left."""
import os
import re

from ogl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The default of every fixed entry as the call sites had it in the commit before the table
# (grep -rhoE 'prop\("[A-Za-z_0-9]+", *[^)]*\)' ogl_amd/csrc | sort -u; FUSED_FIN_MAX_CHUNKS = 1024, HQ_STATIC_DEFAULT = 12
# and MG_TAIL_DEFAULT_ROWS = 512 from kernels.hpp).  No name had two defaults.
FIXED_DEFAULTS = {
    "aggregateCaching": 0.0, "aggregatePasses": 1.0, "aggregation": 0.0, "basisPrecision": 0.0, "bicgFold": 1.0,
    "bicgMergedCheck": 1.0, "bjFusedPerm": 1.0, "bjGroupLanes": 1.0, "bjPermXcdGroup": 0.0, "bjStagedApply": 1.0,
    "coarseSolverIters": 4.0, "coarseVisits": 1.0, "correctionScale": 1.0, "curveOnDevice": 1.0, "cycle": 0.0,
    "cyclePrecision": 0.0, "deferX": 2.0, "deferX2": 1.0, "deviceSetup": 1.0, "factorSweeps": 0.0,
    "fusedFinMaxChunks": 1024.0, "fusedFinalizers": 1.0, "fusedTurn": 1.0, "fusedTurnMulti": 1.0, "gmresFold": 1.0,
    "gmresLead": 0.0, "guessProjection": 0.0, "guessProjectionCredit": 0.0, "guessProjectionProducts": 0.0,
    "guessProjectionTimed": 0.0, "haloFused": 1.0, "heldQIdleGroups": 0.0, "heldQStaticSlots": 12.0, "heldZCensusS": 1.0,
    "heldZEarlySlots": 4.0, "heldZEarlyX": 1.0, "iluThinRows": 256.0, "innerMaxIter": 1000.0, "innerRelTol": 1e-4,
    "isaiGroupLanes": 1.0, "isaiKeepScratch": 0.0, "isaiScratchBytes": 2147483648.0, "isaiSortRows": 1.0,
    "jacobiFromSource": 1.0, "leadEarlyLoads": 1.0, "leadFinalizers": 1.0, "leadTimeoutS": 10.0, "maxLevels": 9.0,
    "mgKeepStream": 0.0, "mgTailRows": 512.0, "minCoarseRows": 10.0, "mixedPrecision": 0.0, "mixedTimedSpmvs": 0.0,
    "orthoMethod": 0.0, "orthoTimedLaunches": 0.0, "precondCallerNumbering": 1.0, "precondTimedApplies": 0.0,
    "renumberCurve": 1.0, "smootherSweeps": 2.0, "spmvBandRows": -1.0, "spmvForceLayout": -1.0, "spmvLdsRounds": 1.0,
    "streamTurnSet": 1.0, "symmetricHalfPerChunk_enable": 1.0, "symmetricHalfWhole_enable": 1.0, "triangularSolves": 0.0,
    "zeroGuess": 1.0,
}
COMPUTED = {"streamAboveBytes", "xcdGroup", "peerSafeWait", "fusedTurnBig", "heldZ", "heldZGrid", "heldZMaxChunks", "heldQ",
            "hipGraph"}
# what the library reads AND writes; the default is what a read found before the first write.  spmvStream is the 83rd
# entry: a report that the ISAI applies read back, and nothing shows that the layout owner's flag always equals it
STATE = {"prevSolveIters": 1.0, "prevSolveIters_final": 1.0, "_prev_solve": 0.0, "preconditionerCaching": 0.0,
         "hipGraphCaptures": 0.0, "guessProjectionReset": 0.0, "spmvStream": 0.0}
# rows of INTEGRATION.md section 6 whose first key is a read-only report
REPORT_ROWS = {"guessProjectionCreditInUse", "guessProjectionOffered", "heldZGridInUse"}


def test_defaults_were_transcribed_not_changed():
    table = capi.property_table()
    assert {n: d for n, d, kind, _ in table if kind == "fixed"} == FIXED_DEFAULTS
    assert {n for n, _, kind, _ in table if kind == "computed"} == COMPUTED
    assert all(d != d for _, d, kind, _ in table if kind == "computed")  # (NaN: the call site has the default)
    assert {n: d for n, d, kind, _ in table if kind == "state"} == STATE
    assert len(table) == len(FIXED_DEFAULTS) + len(COMPUTED) + len(STATE) == 83


def test_names_are_unique_inputs_with_a_text():
    table = capi.property_table()
    names = [n for n, _, _, _ in table]
    assert len(set(names)) == len(names)
    assert not [n for n in names if n.endswith("InUse")]
    assert all(text.strip() for _, _, _, text in table)
    assert capi.lib().ogl_host_property(len(table), None, None, None, None) == capi.ERR_INVALID
    assert capi.lib().ogl_host_property(-1, None, None, None, None) == capi.ERR_INVALID


def test_every_entry_has_a_row_in_the_integration_guide():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        section = f.read().split("\n## 6. Properties", 1)[1]
    rows = re.findall(r"^\| `([A-Za-z_0-9]+)`", section, re.M)
    names = {n for n, _, _, _ in capi.property_table()}
    assert names - set(rows) == set()
    assert set(rows) - names == REPORT_ROWS
    assert len(rows) == len(set(rows))


def test_no_property_is_read_by_string():
    src = os.path.join(ROOT, "ogl_amd", "csrc")
    hits = []
    for name in sorted(os.listdir(src)):
        with open(os.path.join(src, name)) as f:
            hits += [f"{name}:{i}" for i, line in enumerate(f, 1) if 'prop("' in line]
    assert hits == []
