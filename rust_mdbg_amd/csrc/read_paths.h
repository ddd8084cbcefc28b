// read_paths.h — interface between the C ABI (graph_api.inc) and the read-path translation unit (read_paths.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_read_paths).  The windows are placed by the placement unit (placement.h), in the context's one placement scratch.
#pragma once
#include "placement.h"

struct ReadPathBuffers;            // scratch + results, owned by the context (opaque here)
ReadPathBuffers* read_path_buffers_create();
void read_path_buffers_destroy(ReadPathBuffers*);

struct ReadPathResult {            // device pointers into ReadPathBuffers, valid until the next call
    uint64_t n_reads, n_windows, n_placed, n_steps, n_unitigs;
    const uint64_t* ordinal; const uint32_t* read_windows; const uint64_t* step_offsets;
    const uint32_t* first_window; const uint32_t* step_windows; const uint32_t* unitig; const uint32_t* first_entry; const uint8_t* strand;
    const uint64_t* support_windows; const uint64_t* support_steps;
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_*; ms: device time of the call, from its first memset to its last kernel
};
// One call: grows every buffer, queues the zeroing, the placement (placement_queue, which calls the placer) and the rest (head flags, one scan, the steps, the
// sums), reads the counters back and waits ONCE.  Every launch count is fixed.
// The three parts of that call, for a stage that goes on from the steps on the device (alignments.hip): read_paths_reserve grows every buffer (the placement's
// included, with or without records); read_paths_queue queues the zeroing, the placement and the read-path kernels and fills *out's pointers and n_reads / n_unitigs,
// *view and the scratch the steps were numbered with (flag[t] = 1 iff index t starts a step, pos = its exclusive scan), and waits for nothing; read_paths_counts
// fills the counts and the defect mask from the counter block once the caller has read it back.  The caller owns the timer and the one wait.
struct ReadPathScratch { const uint8_t* flag; const uint32_t* pos; };
hipError_t read_paths_reserve(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, uint64_t n_rows, const ReadPathRange& rg, bool with_records);
hipError_t read_paths_queue(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, bool with_records,
                            uint32_t n_counters, const WindowPlacer& placer, hipStream_t s, PlacementView* view, ReadPathResult* out, ReadPathScratch* scratch);
void read_paths_counts(const uint64_t* counters, ReadPathResult* out);
hipError_t read_paths_run(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, const WindowPlacer& placer,
                          hipStream_t s, ReadPathResult* out);
