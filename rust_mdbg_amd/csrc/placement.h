// placement.h — where on the current unitig list every resident window lies, and the sorted keys of the list's edge records: the first half of every stage that
// decides with the resident reads (read_paths.hip, junctions.hip, transits.hip, the EDGES step of simplify.hip).  The scratch is the context's, once
// (PlacementBuffers, placement.hip); place_windows_kernel itself lives in the main translation unit beside the table (place_windows.hip) and is reached through
// a WindowPlacer only.  Nothing here is a result: every call of a stage overwrites it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unitigs.h"

struct PlacementBuffers;           // scratch, owned by the context (opaque here)
PlacementBuffers* placement_buffers_create();
void placement_buffers_destroy(PlacementBuffers*);

constexpr uint32_t RP_NONE = 0xFFFFFFFFu;         // entry_of_row: the row is in no entry; code: no window starts at the index, or the window is not placed
constexpr uint32_t RP_STRAND = 0x80000000u;       // code = entry | strand << 31 (a list has fewer than 2^30 entries)
// On a list that holds copies (include/mdbg_hip.h, MDBG_SIMPLIFY_NESTED: placement on a list that holds copies) a window whose row belongs to several entries
// first gets an AMBIGUOUS code, row | RP_AMBIGUOUS | rev << 31: bit 30 is free because entries and rows are both below 2^30, and rows end below 2^30 - 1, so
// no such code is RP_NONE.  resolve_kernel (placement.hip) rewrites every one of them to the format above or to RP_NONE before a stage reads code[].
constexpr uint32_t RP_AMBIGUOUS = 0x40000000u;
// the copies of the schedule so far: node index X + c, c < copies, descends from the table row with index origin[c].  copies == 0: the list holds none
struct OriginMap { uint32_t X; uint64_t copies; const uint32_t* origin; };
constexpr OriginMap NO_COPIES = {0, 0, nullptr};
// counters[] (u64 each), one read-back per call: the placement's own first, a stage's behind them (JX_C_*, TX_C_*).  RP_C_DEFECT is a mask of RP_DEFECT_*
enum { RP_C_WINDOWS = 0, RP_C_PLACED, RP_C_STEPS, RP_C_DEFECT, RP_C_N };
constexpr uint32_t PLACEMENT_COUNTERS = 16;       // the size of the block: it holds the largest stage's counters (each stage asserts that)
// with copies, the last four of the block: the ambiguous windows, those placed by an anchor (counted in RP_C_PLACED too), those whose two anchors disagree, and
// those without a valid candidate.  ambiguous == resolved + conflicts + unanchored
enum { NP_C_AMBIGUOUS = PLACEMENT_COUNTERS - 4, NP_C_RESOLVED, NP_C_CONFLICTS, NP_C_UNANCHORED };
enum { RP_DEFECT_ENTRY = 1,        // a list entry whose node index is not a row of the table
       RP_DEFECT_PROBE = 2,        // a probe sequence visited every slot of the table
       RP_DEFECT_ROW = 4 };        // a solid slot whose first sighting is no row of the table (the bitmaps are not this table's)
constexpr uint32_t JX_DEFECT_EDGE = 8;            // beside RP_DEFECT_*: an edge record names a unitig outside the list (record_key_kernel)

// the reads [first_read, first_read + n_reads) of the store and the minimizer indices [i0, i1) they cover
struct ReadPathRange {
    const uint64_t* roff; const uint32_t* mread; uint32_t first_read, n_reads, k; uint64_t i0, i1;
    const uint32_t* by_slot0; const uint64_t* by_slot_first; uint32_t n_batches;      // the batches in slot order: first slot, first ordinal; n_batches == 0: a range that is in no batch table (a temporary batch), ordinal = the read's number in the range
};
// what place_windows_kernel reads and writes beside the table and the store
struct ReadPathPlan {
    const uint32_t* entry_of_row; uint64_t n_rows; const uint8_t* ori;
    uint32_t* code;                // [i1 - i0]
    uint64_t* counters;            // [PLACEMENT_COUNTERS]
    const uint32_t* mult;          // [n_rows] with copies: the entries of the list per row (a row with two or more gets an ambiguous code); else null
};
// launches place_windows_kernel for the plan on the stream (graph_api.inc has the one there is)
struct WindowPlacer { void (*place)(void* ctx, const ReadPathPlan& plan, hipStream_t s); void* ctx; };
// what placement_queue leaves for the stage's kernels, valid until the next call of any stage
struct PlacementView {
    const uint32_t* entry_of_row;  // [n_rows]
    const uint32_t* unitig_of_entry;      // [n_entries]
    const uint32_t* code;          // [i1 - i0]: global entry | strand << 31, or RP_NONE
    uint64_t* counters;            // [PLACEMENT_COUNTERS]
    const uint64_t* rkey_sorted; const uint32_t* rec_sorted; uint64_t R;      // with records: the R edge records in key order (stable: a key's run starts at its smallest record)
};
// (with copies entry_of_row[r] is an entry of row r, meaningful where mult[r] == 1 only; no stage reads it)
// placement_reserve checks the bounds (hipErrorInvalidValue: the caller has answered MDBG_E_CAPACITY or returned before) and grows every buffer of the unit,
// the sort's temporary included; a stage calls it beside its own `ensure`s, before it queues anything.  placement_queue then grows nothing: it queues the zeroing
// of the first n_counters counters and of the map, entry_kernel, with records record_key_kernel and the stable pair sort, and the placer, and fills *view.
// om.copies > 0 (both calls get the same map): the list holds copies.  The reserve grows four more blocks; the queue zeroes mult and the last four counters too,
// runs the entry kernel's instantiation that maps a copy's index to its origin, and behind the placer mark_kernel, two max-scans and resolve_kernel: a fixed
// number of launches, and code[] is in the plain format when the stage's kernels start.
hipError_t placement_reserve(PlacementBuffers* P, const UnitigResult& ul, uint64_t n_rows, const ReadPathRange& rg, bool with_records, const OriginMap& om = NO_COPIES);
hipError_t placement_queue(PlacementBuffers* P, const UnitigResult& ul, const uint32_t* index, uint64_t n_rows, const ReadPathRange& rg, bool with_records, uint32_t n_counters,
                           const WindowPlacer& placer, hipStream_t s, PlacementView* view, const OriginMap& om = NO_COPIES);
// the record keys in key order as the last placement_queue WITH records left them, for a stage that runs behind another stage's call and reads what it left on the
// device (chains.hip behind alignments_run); R is the list's edges.n.  Valid until the next call of any stage.
void placement_records(const PlacementBuffers* P, const uint64_t** rkey_sorted, const uint32_t** rec_sorted);
