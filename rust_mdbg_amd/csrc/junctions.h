// junctions.h — interface between the C ABI (graph_api.inc) and the junction translation unit (junctions.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_junctions).  The windows are placed and the edge records keyed by the placement unit (placement.h), in the context's one placement scratch.
#pragma once
#include "placement.h"

struct JunctionBuffers;            // scratch + results, owned by the context (opaque here)
JunctionBuffers* junction_buffers_create();
void junction_buffers_destroy(JunctionBuffers*);

// counters[] (u64 each), one read-back per call: the placement's counters first (place_windows_kernel writes them), the stage's own behind them
enum { JX_C_ADJACENT = RP_C_N, JX_C_LINKS, JX_C_EXPLAINED, JX_C_MISSING_CROSSINGS, JX_C_MISSING, JX_C_N };
static_assert(JX_C_N <= NP_C_AMBIGUOUS, "the placement's counter block holds every stage's counters");

struct JunctionResult {            // device pointers into JunctionBuffers, valid until the next call
    uint64_t n_reads, n_adjacent, n_links, n_crossings, n_explained, n_missing_crossings, n_records, n_missing;
    const uint64_t* support;                                                                       // n_records
    const uint32_t* missing_unitig1; const uint32_t* missing_entry1; const uint8_t* missing_strand1;     // n_missing each
    const uint32_t* missing_unitig2; const uint32_t* missing_entry2; const uint8_t* missing_strand2;
    const uint64_t* missing_count;
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_* | JX_DEFECT_EDGE; ms: device time of the call, from its first memset to its last kernel
};
// One call: grows every buffer, queues the zeroing, the placement with the sorted record keys (placement_queue, which calls the placer) and the rest (the
// crossings, one sort, one scan, the missing list, the supports), reads the counters back and waits ONCE.  Every launch count is fixed.
// om: the copies the list holds (placement.h); no caller passes one yet, an EDGES step behind a step that copied is refused.
hipError_t junctions_run(JunctionBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, const WindowPlacer& placer,
                         hipStream_t s, JunctionResult* out, const OriginMap& om = NO_COPIES);
