// contigs.h — interface between the C ABI (api.inc) and the contig-stitching translation unit (contigs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edges.h"
#include "unitigs.h"

// One kept batch of the resident read store (MDBG_FLAG_KEEP_READS), in the packed layout of mdbg_packed_batch: all pointers DEVICE memory.
// The stitch kernel gets a table of these sorted by first_ordinal and finds the batch of a read ordinal by binary search.
struct KeptDesc {
    uint64_t first_ordinal, n_reads;
    const uint2* planes; uint64_t n_words;           // two 32-bit planes per 32 bases
    const uint64_t* offsets;                         // n_reads + 1, in bases into the planes
    const uint64_t* exc_pos; const uint8_t* exc_val; uint64_t n_exc;      // bytes outside ACGT, ascending by position
};

struct ContigBuffers;              // scratch + results, owned by the context (opaque here)
ContigBuffers* contig_buffers_create();
void contig_buffers_destroy(ContigBuffers*);

struct ContigResult {              // device pointers into ContigBuffers, valid until the next stitch_contigs
    uint64_t n_contigs, n_bases;
    const uint8_t* bases; const uint64_t* offsets; const uint64_t* unitig;
    uint32_t err;                  // bit 0: a plan entry names a read that is not kept; bit 1: a plan entry lies outside its read
    float ms_stitch;               // device time of the stitch kernel alone (HIP events)
};
// Executes the copy plan of `ul` (the unitigs with length >= min_len, in list order) against the kept batches `tab` (HOST array, sorted by first_ordinal).
// Returns hipSuccess (look at out->err) or the failing HIP error.  Synchronises the stream before returning.
hipError_t stitch_contigs(ContigBuffers* B, const UnitigResult& ul, const KeptDesc* tab, uint32_t n_tab, uint64_t min_len, hipStream_t s, ContigResult* out);

// the exception side-list as pack_planes_kernel leaves it (unordered) -> ascending by position (rocPRIM radix sort of (position, byte) pairs; stream-ordered)
hipError_t sort_exceptions(ContigBuffers* B, const uint64_t* pos_in, const uint8_t* val_in, uint64_t* pos_out, uint8_t* val_out, uint64_t n, hipStream_t s);
