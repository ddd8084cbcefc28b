// read_paths.h — interface between the C ABI (api.inc), the window-placing kernel of the main translation unit (place_windows.hip) and the read-path
// translation unit (read_paths.hip).  Definition: include/mdbg_hip.h (mdbg_graph_read_paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unitigs.h"

struct ReadPathBuffers;            // scratch + results, owned by the context (opaque here)
ReadPathBuffers* read_path_buffers_create();
void read_path_buffers_destroy(ReadPathBuffers*);

constexpr uint32_t RP_NONE = 0xFFFFFFFFu;         // entry_of_row: the row is in no entry; code: no window starts at the index, or the window is not placed
constexpr uint32_t RP_STRAND = 0x80000000u;       // code = entry | strand << 31 (a list has fewer than 2^30 entries)
// counters[] (u64 each), one read-back per call.  RP_C_DEFECT is a mask of RP_DEFECT_*
enum { RP_C_WINDOWS = 0, RP_C_PLACED, RP_C_STEPS, RP_C_DEFECT, RP_C_N };
enum { RP_DEFECT_ENTRY = 1,        // a list entry whose node index is not a row of the table
       RP_DEFECT_PROBE = 2,        // a probe sequence visited every slot of the table
       RP_DEFECT_ROW = 4 };        // a solid slot whose first sighting is no row of the table (the bitmaps are not this table's)

// the reads [first_read, first_read + n_reads) of the store and the minimizer indices [i0, i1) they cover
struct ReadPathRange {
    const uint64_t* roff; const uint32_t* mread; uint32_t first_read, n_reads, k; uint64_t i0, i1;
    const uint32_t* by_slot0; const uint64_t* by_slot_first; uint32_t n_batches;      // the batches in slot order: first slot, first ordinal
};
// what place_windows_kernel reads and writes beside the table and the store
struct ReadPathPlan {
    const uint32_t* entry_of_row; uint64_t n_rows; const uint8_t* ori;
    uint32_t* code;                // [i1 - i0]
    uint64_t* counters;            // [RP_C_N]
};
struct ReadPathResult {            // device pointers into ReadPathBuffers, valid until the next call
    uint64_t n_reads, n_windows, n_placed, n_steps, n_unitigs;
    const uint64_t* ordinal; const uint32_t* read_windows; const uint64_t* step_offsets;
    const uint32_t* first_window; const uint32_t* step_windows; const uint32_t* unitig; const uint32_t* first_entry; const uint8_t* strand;
    const uint64_t* support_windows; const uint64_t* support_steps;
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_*; ms: device time from read_paths_begin to the end of read_paths_end
};
// The placement half, which the junction stage (junctions.hip) shares: the arrays belong to the caller's stage.  placement_begin queues the zeroing of the
// first n_counters counters (>= RP_C_N: a stage may keep counts of its own behind them) and of the map, and entry_kernel, and fills *plan; place_windows_kernel,
// launched by the caller on the same stream, then writes code[] and the counters RP_C_WINDOWS, RP_C_PLACED and RP_C_DEFECT.
struct PlacementArrays {
    uint32_t* entry_of_row;        // [n_rows]
    uint32_t* unitig_of_entry;     // [n_entries]
    uint32_t* code;                // [i1 - i0]
    uint64_t* counters; uint32_t n_counters;
};
hipError_t placement_begin(const PlacementArrays& A, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, hipStream_t s, ReadPathPlan* plan);
// read_paths_begin queues the zeroing and the row -> entry map and fills *plan; the caller then launches place_windows_kernel on the same stream;
// read_paths_end queues the rest (head flags, one scan, the steps, the sums), reads the counters back and waits ONCE.  Every launch count is fixed.
hipError_t read_paths_begin(ReadPathBuffers* B, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, hipStream_t s, ReadPathPlan* plan);
hipError_t read_paths_end(ReadPathBuffers* B, const UnitigResult& ul, const ReadPathRange& rg, hipStream_t s, ReadPathResult* out);
