// junctions.h — interface between the C ABI (graph_api.inc) and the junction translation unit (junctions.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_junctions).  The stage places the windows as the read paths do (read_paths.h: placement_begin, place_windows_kernel), in buffers of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "read_paths.h"

struct JunctionBuffers;            // scratch + results, owned by the context (opaque here)
JunctionBuffers* junction_buffers_create();
void junction_buffers_destroy(JunctionBuffers*);

// counters[] (u64 each), one read-back per call: the read paths' counters first (place_windows_kernel writes them), the stage's own behind them
enum { JX_C_ADJACENT = RP_C_N, JX_C_LINKS, JX_C_EXPLAINED, JX_C_MISSING_CROSSINGS, JX_C_MISSING, JX_C_N };
constexpr uint32_t JX_DEFECT_EDGE = 8;      // beside RP_DEFECT_*: an edge record names a unitig outside the list

struct JunctionResult {            // device pointers into JunctionBuffers, valid until the next call
    uint64_t n_reads, n_adjacent, n_links, n_crossings, n_explained, n_missing_crossings, n_records, n_missing;
    const uint64_t* support;                                                                       // n_records
    const uint32_t* missing_unitig1; const uint32_t* missing_entry1; const uint8_t* missing_strand1;     // n_missing each
    const uint32_t* missing_unitig2; const uint32_t* missing_entry2; const uint8_t* missing_strand2;
    const uint64_t* missing_count;
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_* | JX_DEFECT_EDGE; ms: device time from junctions_begin to the end of junctions_end
};
// junctions_begin queues the zeroing, the row -> entry map and the sorted record keys and fills *plan; the caller then launches place_windows_kernel on the same
// stream; junctions_end queues the rest (the crossings, one sort, one scan, the missing list, the supports), reads the counters back and waits ONCE.
// Every launch count is fixed.
hipError_t junctions_begin(JunctionBuffers* B, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, hipStream_t s, ReadPathPlan* plan);
hipError_t junctions_end(JunctionBuffers* B, const UnitigResult& ul, const ReadPathRange& rg, hipStream_t s, JunctionResult* out);
