// chains.h — interface between the C ABI (graph_api.inc) and the chain translation unit (chains.hip).  Definition: include/mdbg_chain.h (mdbg_graph_chains).
// The stage runs BEHIND alignments_run and reads what that call left on the device: the steps (read_paths.h), the alignments (alignments.h) and the sorted record
// keys of the placement (placement_records, placement.h).
#pragma once
#include "alignments.h"

struct ChainBuffers;               // scratch + results, owned by the context (opaque here)
ChainBuffers* chain_buffers_create();
void chain_buffers_destroy(ChainBuffers*);

constexpr uint32_t CH_INSIDE = 0xFFFFFFFEu;       // bridge_record of an INSIDE bridge; RP_NONE (0xFFFFFFFF): not bridged

struct ChainResult {               // device pointers into ChainBuffers, valid until the next call
    uint64_t n_bridges_inside, n_bridges_record, n_gap_windows, n_chains;
    const uint32_t* bridge_record; const uint64_t* bridge_entries;                           // n_alignments
    const uint64_t* chain_offsets;                                                           // n_reads + 1
    const uint64_t* chain_aln_offsets;                                                       // n_chains + 1
    const uint32_t* chain_windows; const uint32_t* chain_gap_windows; const uint32_t* query_begin; const uint32_t* query_end;      // n_chains
    const uint64_t* path_length; const uint64_t* path_begin; const uint64_t* path_end;      // n_chains
    uint32_t defect; float ms;     // defect: AL_DEFECT_RECORD (a step, unitig or record an alignment names lies outside its list); ms: device time of this stage alone
};
// One call behind alignments_run of the same range, whose counts the host has: grows every buffer (sized by n_alignments), queues five memsets (one of them the single byte head[n_alignments]), bridge_kernel, one
// scan, chain_sum_kernel, chain_coord_kernel and chain_reads_kernel, reads the counters back and waits ONCE.  l: the context's minimizer length (the base overlap of a record).
hipError_t chains_run(ChainBuffers* C, const PlacementBuffers* P, const UnitigResult& ul, const ReadPathResult& rp, const AlignmentResult& al, uint32_t l,
                      uint32_t max_skew, uint32_t max_gap, hipStream_t s, ChainResult* out);
