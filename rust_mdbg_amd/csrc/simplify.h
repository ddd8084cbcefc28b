// simplify.h — interface between the C ABI (api.inc) and the simplification stage (simplify.hip).
#pragma once
#include "../../include/mdbg_hip.h"
#include "components.h"
#include "junctions.h"
#include "transits.h"
#include "unitigs.h"

// the defect mask of a REPEATS step (repeats.hip)
constexpr uint32_t RX_DEFECT_MATCH = 1;     // an end of an edge record at a resolved unitig belongs to no strong key, or to two
constexpr uint32_t RX_DEFECT_SHAPE = 2;     // a vertex of the last compaction lies outside the list, or a transit row outside its unitig
struct SimplifyInfo { uint32_t n_compactions, n_rounds_total, n_syncs, junction_defect; float junction_ms;      // compactions run, their jumping rounds, host synchronisations of the whole call; of the EDGES steps' junction stages: the defect mask (*broken is set with it) and the device time, summed
                      uint32_t transit_defect, repeats_defect; bool repeats_too_large; float transit_ms; uint64_t copies;      // of the REPEATS and NESTED steps: the transit stage's defect mask and their own (RX_DEFECT_*; *broken is set with either), the capacity refusal (*broken is set too), the transit stages' device time, the entries the schedule copied
                      uint64_t ambiguous, resolved, conflicts, unanchored; };      // of the NESTED steps on a graph with copies, summed: the windows whose row belongs to several entries and what became of them (placement.h, NP_C_*)
// What an MDBG_SIMPLIFY_EDGES step needs beside the graph to run the junction stage (junctions_run): that stage's buffers and the context's placement scratch, the
// node table's index column, the whole resident store as a range of reads, and the window placer.  has_reads == false: nothing is resident, every record is weak.
// An MDBG_SIMPLIFY_REPEATS or MDBG_SIMPLIFY_NESTED step needs the same with the transit stage's buffers (transits_run) in place of the junction stage's; nothing resident: nothing resolves.
struct SimplifySupport {
    JunctionBuffers* jb; TransitBuffers* tb; PlacementBuffers* pb; const uint32_t* index; uint64_t n_rows; ReadPathRange range; bool has_reads; WindowPlacer placer;
};
// Runs the schedule on the node table and edge list (mdbg_graph_simplify, include/mdbg_hip.h) and leaves the unitig list of the surviving graph in *out, in
// the same buffers as build_unitigs (valid until the next call of either).  unitigs_removed / nodes_removed / edges_removed: n_steps host entries.  Return value and *broken as build_unitigs.
// CB: the component stage's buffers, used by MDBG_SIMPLIFY_COMPONENTS steps (may be null when the schedule has none); sup: the same for MDBG_SIMPLIFY_EDGES and MDBG_SIMPLIFY_REPEATS steps.
hipError_t simplify_unitigs(UnitigBuffers* B, ComponentBuffers* CB, const SimplifySupport* sup, const UnitigNodes& nd, const EdgeResult& ed, const mdbg_simplify_step* steps, uint32_t n_steps,
                     hipStream_t s, UnitigResult* out, uint64_t* unitigs_removed, uint64_t* nodes_removed, uint64_t* edges_removed, SimplifyInfo* info, int* broken);
