// node_seqs.h — interface between the C ABI (graph_api.inc) and the node-sequence translation unit (node_seqs.hip): the bases of the node table's rows,
// gathered out of the resident read store in bounded chunks (mdbg_graph_node_seqs, include/mdbg_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "contigs.h"

struct NodeSeqBuffers;             // the cached prefix, scratch and the last chunk: owned by the context (opaque here); nothing is shared with ContigBuffers
NodeSeqBuffers* node_seq_buffers_create();
void node_seq_buffers_destroy(NodeSeqBuffers*);

struct NodeSeqRows {               // device columns of the node table (finalize's rows), n rows
    const uint64_t* src_read; const uint64_t* src_start; const uint64_t* src_end; const uint8_t* reversed; uint64_t n;
};
struct NodeSeqResult {             // device pointers into NodeSeqBuffers, valid until the next node_seq_chunk
    uint64_t first_row, n_rows, n_bases;
    const uint8_t* bases; const uint64_t* offsets;
    uint32_t err;                  // bit 0: a row names a read that is not kept; bit 1: a row lies outside its read
    float ms_gather;               // device time of the gather kernel alone (HIP events; 0 when no base was produced)
};
// Once per node table: prefix[i] = sum of src_end - src_start over the rows before i (n + 1 entries), kept in B until the next call.  Stream-ordered, no host wait.
hipError_t node_seq_prefix(NodeSeqBuffers* B, const NodeSeqRows& rows, hipStream_t s);
// Rows [first_row, first_row + n_rows) with n_rows the largest count <= max_rows whose bases are <= max_bases (0: no limit; at least one row while
// first_row < rows.n).  `tab`: the kept batches, HOST array sorted by first_ordinal.  Needs the prefix of the same rows.  Waits for the stream twice at most
// (the chunk's size, the error flag).  Returns hipSuccess (look at out->err) or the failing HIP error.
hipError_t node_seq_chunk(NodeSeqBuffers* B, const NodeSeqRows& rows, const KeptDesc* tab, uint32_t n_tab, uint64_t first_row, uint64_t max_rows, uint64_t max_bases,
                          hipStream_t s, NodeSeqResult* out);
