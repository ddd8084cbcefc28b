// transits.h — interface between the C ABI (graph_api.inc) and the transit translation unit (transits.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_transits).  The windows are placed and the edge records keyed by the placement unit (placement.h), in the context's one placement scratch.
#pragma once
#include "placement.h"

struct TransitBuffers;             // scratch + results, owned by the context (opaque here)
TransitBuffers* transit_buffers_create();
void transit_buffers_destroy(TransitBuffers*);

// counters[] (u64 each), one read-back per call: the placement's counters first (place_windows_kernel writes them), the stage's own behind them
enum { TX_C_ADJACENT = RP_C_N, TX_C_LINKS, TX_C_EXPLAINED, TX_C_PASSES, TX_C_TRANSITS, TX_C_REPEATS, TX_C_RESOLVED, TX_C_N };
static_assert(TX_C_N <= NP_C_AMBIGUOUS, "the placement's counter block holds every stage's counters");
constexpr uint32_t TX_DEFECT_SHAPE = 16;    // beside RP_DEFECT_* and JX_DEFECT_EDGE: a chain of two explained crossings that does not walk all of one unitig

struct TransitResult {             // device pointers into TransitBuffers, valid until the next call
    uint64_t n_reads, n_crossings, n_explained, n_passes, n_transits, n_unitigs, n_repeats, n_resolved;
    const uint32_t* unitig;                                                                        // n_transits each
    const uint32_t* in_unitig; const uint32_t* in_entry; const uint8_t* in_strand;
    const uint32_t* out_unitig; const uint32_t* out_entry; const uint8_t* out_strand;
    const uint32_t* in_record; const uint32_t* out_record; const uint64_t* count;
    const uint32_t* n_in; const uint32_t* n_out; const uint64_t* passes; const uint8_t* verdict;   // n_unitigs each
    uint64_t ambiguous, resolved, conflicts, unanchored;      // with copies (NP_C_* of placement.h): the windows whose row belongs to several entries, and what became of them
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_* | JX_DEFECT_EDGE | TX_DEFECT_SHAPE; ms: device time of the call, from its first memset to its last kernel
};
// One call: grows every buffer, queues the zeroing, the placement with the sorted record keys (placement_queue, which calls the placer) and the rest (the
// events, one scan, the keys, two sorts, one scan, the rows, the verdicts), reads the counters back and waits ONCE.  Every launch count is fixed.
// om: the copies the list holds (placement.h).  With copies the placement takes five more launches (one kernel, two scans, one kernel, and two memsets), the
// read-back carries the four counts of the ambiguous windows, and the wait is still the one.
hipError_t transits_run(TransitBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, uint64_t min_support,
                        const WindowPlacer& placer, hipStream_t s, TransitResult* out, const OriginMap& om = NO_COPIES);
