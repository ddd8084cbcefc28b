// repeats.h — interface between the simplification stage (simplify.hip) and the REPEATS step's translation unit (repeats.hip).  Definition: include/mdbg_hip.h
// (mdbg_graph_simplify, MDBG_SIMPLIFY_REPEATS).  Included by those two translation units only (it shows the compaction's buffers, unitigs_priv.h).
#pragma once
#include "simplify.h"
#include "transits.h"
#include "unitigs_priv.h"

struct RepeatsResult {             // device pointers into UnitigBuffers (the x_* blocks), valid until the next REPEATS or NESTED step
    UnitigNodes nd; EdgeResult ed;          // the extended node columns and edge records: the originals keep their rows and record numbers, the copies are appended
    uint8_t* alive; uint8_t* edge_alive;    // the extended masks (edge_alive: null if the step was given none)
    uint64_t copies, records_added;         // of this step
    uint64_t total_copies;                  // of the schedule so far, this step included
    uint32_t first_copy_index;              // X = 1 + the table's largest index: copy c of the schedule has index X + c
    const uint32_t* origin;                 // [total_copies]: the index of the table row a copy descends from
    uint32_t defect; bool too_large;        // defect: mask of RX_DEFECT_* (simplify.h); too_large: 2^30 rows or 2^32 records would be reached (nothing was copied)
};
// The step on the list `ul` of the last compaction in B (whose arrays it reads: eu / ev / ekeep, the settled ranking, uid, hoff) and the transit result of that
// list.  tr.n_resolved > 0 and ed.n > 0 are the caller's business.  Queues three kernels and three scans, reads the three totals back (the first wait), grows the
// x_* blocks, queues the copies of the originals' columns and two more kernels, and reads the defect flag back (the second wait).  Every launch count is fixed.
// table_last_index: the device address of the node TABLE's largest index (its last row).  earlier: the result of the schedule's last step that copied, or null;
// with it nd, ed and the masks live in the x_* blocks, the step grows into fresh blocks and swaps them in, and origin[] goes on behind the earlier copies.
// out must not be earlier.  A step that returns an error or is refused as too large leaves the x_* blocks as they were.  A step that ran to its end and reports a
// defect (out->defect != 0) has swapped the new blocks in like any other: out names them, and the caller ends the schedule as broken.
hipError_t repeats_run(UnitigBuffers* B, const TransitResult& tr, uint64_t min_support, const UnitigResult& ul, const UnitigNodes& nd, const EdgeResult& ed, const uint8_t* alive,
                       const uint8_t* edge_alive, const uint32_t* table_last_index, const RepeatsResult* earlier, hipStream_t s, RepeatsResult* out);
// node[] of the list in B: a copy's index -> its original's (one kernel, no wait)
hipError_t repeats_report_originals(UnitigBuffers* B, const UnitigResult& ul, const RepeatsResult& r, hipStream_t s);
