// alignments.h — interface between the C ABI (graph_api.inc) and the alignment translation unit (alignments.hip).  Definition: include/mdbg_align.h
// (mdbg_graph_alignments).  The steps are the read-path unit's (read_paths.h), in ITS buffers: the call fills the context's read-path result too.
#pragma once
#include "read_paths.h"

struct AlignmentBuffers;           // scratch + results, owned by the context (opaque here)
AlignmentBuffers* alignment_buffers_create();
void alignment_buffers_destroy(AlignmentBuffers*);

// counters[] behind the placement's own (placement.h)
enum { AL_C_CHAINED = RP_C_N, AL_C_ALIGNMENTS, AL_C_WRAPS, AL_C_N };
static_assert(AL_C_N <= NP_C_AMBIGUOUS, "the placement's counter block holds every stage's counters");
// beside RP_DEFECT_*, JX_DEFECT_EDGE and TX_DEFECT_SHAPE (16): a record that is needed is absent or outside the list (the closing record of a ring a step
// wraps, the record of a chained step), or a window of an alignment reaches past the range
constexpr uint32_t AL_DEFECT_RECORD = 32;

// the rows of the node table the coordinates need, and the store's raw positions
struct AlignmentNodes { const uint32_t* index; const uint64_t* src_start; const uint64_t* src_end; uint64_t n_rows; const uint32_t* positions; uint32_t l; };

struct AlignmentResult {           // device pointers into AlignmentBuffers, valid until the next call
    uint64_t n_chained, n_alignments, n_wraps;
    const uint64_t* aln_offsets;           // n_reads + 1
    const uint64_t* aln_step_offsets;      // n_alignments + 1
    const uint32_t* step_record;           // n_steps
    const uint32_t* aln_windows; const uint32_t* query_begin; const uint32_t* query_end;      // n_alignments
    const uint64_t* path_length; const uint64_t* path_begin; const uint64_t* path_end;       // n_alignments
    uint32_t defect; float ms;     // defect: mask of RP_DEFECT_* | JX_DEFECT_EDGE | AL_DEFECT_RECORD; ms: device time of the call, from its first memset to its last kernel
};
// One call: grows every buffer, queues the read-path stage over a placement WITH records (read_paths_queue) and the five launches of its own behind it, reads
// the counters back and waits ONCE.  *rp is the read-path result of the range, *out the alignments.  Every launch count is fixed.
hipError_t alignments_run(AlignmentBuffers* A, ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const AlignmentNodes& nd, const ReadPathRange& rg,
                          const WindowPlacer& placer, hipStream_t s, ReadPathResult* rp, AlignmentResult* out);
