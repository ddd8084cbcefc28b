// transits.h — interface between the C ABI (graph_api.inc) and the transit translation unit (transits.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_transits).  The stage places the windows as the read paths do (read_paths.h: placement_begin, place_windows_kernel) and keys the edge records as
// the junction stage does (record_keys.h), in buffers of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "junctions.h"

struct TransitBuffers;             // scratch + results, owned by the context (opaque here)
TransitBuffers* transit_buffers_create();
void transit_buffers_destroy(TransitBuffers*);

// counters[] (u64 each), one read-back per call: the read paths' counters first (place_windows_kernel writes them), the stage's own behind them
enum { TX_C_ADJACENT = RP_C_N, TX_C_LINKS, TX_C_EXPLAINED, TX_C_PASSES, TX_C_TRANSITS, TX_C_REPEATS, TX_C_RESOLVED, TX_C_N };
constexpr uint32_t TX_DEFECT_SHAPE = 16;    // beside RP_DEFECT_* and JX_DEFECT_EDGE: a chain of two explained crossings that does not walk all of one unitig

struct TransitResult {             // device pointers into TransitBuffers, valid until the next call
    uint64_t n_reads, n_crossings, n_explained, n_passes, n_transits, n_unitigs, n_repeats, n_resolved;
    const uint32_t* unitig;                                                                        // n_transits each
    const uint32_t* in_unitig; const uint32_t* in_entry; const uint8_t* in_strand;
    const uint32_t* out_unitig; const uint32_t* out_entry; const uint8_t* out_strand;
    const uint32_t* in_record; const uint32_t* out_record; const uint64_t* count;
    const uint32_t* n_in; const uint32_t* n_out; const uint64_t* passes; const uint8_t* verdict;   // n_unitigs each
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_* | JX_DEFECT_EDGE | TX_DEFECT_SHAPE; ms: device time from transits_begin to the end of transits_end
};
// transits_begin queues the zeroing, the row -> entry map and the sorted record keys and fills *plan; the caller then launches place_windows_kernel on the same
// stream; transits_end queues the rest (the events, one scan, the keys, two sorts, one scan, the rows, the verdicts), reads the counters back and waits ONCE.
// Every launch count is fixed.
hipError_t transits_begin(TransitBuffers* B, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, hipStream_t s, ReadPathPlan* plan);
hipError_t transits_end(TransitBuffers* B, const UnitigResult& ul, const ReadPathRange& rg, uint64_t min_support, hipStream_t s, TransitResult* out);
