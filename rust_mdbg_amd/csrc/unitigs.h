// unitigs.h — interface between the C ABI (api.inc) and the unitig-compaction translation unit (unitigs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edges.h"

struct UnitigNodes {               // device-resident node table of the last finalize (rows in index order): the columns compaction and the copy plan read
    const uint32_t* index; const uint16_t* abund; const uint64_t* shift_full; const uint64_t* src_read; const uint64_t* src_start; const uint64_t* src_end;
    const uint8_t* reversed; uint64_t n;
};
struct UnitigBuffers;              // scratch + results, owned by the context (opaque here)
UnitigBuffers* unitig_buffers_create();
void unitig_buffers_destroy(UnitigBuffers*);

struct UnitigResult {              // device pointers into UnitigBuffers, valid until the next call
    uint64_t n_unitigs, n_entries;
    const uint64_t* offsets; const uint32_t* node; const uint8_t* ori;
    const uint64_t* src_read; const uint64_t* src_begin; const uint32_t* len; const uint8_t* revcomp; const uint64_t* dst_offset;
    const uint64_t* length; const uint64_t* kc_sum; const uint8_t* circular;
    EdgeResult edges;              // unitig edges (n1 / n2 = 0-based unitig numbers)
    uint32_t n_rounds;             // pointer-jumping rounds this call ran
};
// Returns hipSuccess or the failing HIP error.  *broken <- 1 (with hipSuccess, *out empty) when the jumping did not converge within its bound or an invariant of
// the walk does not hold (a defect, never the input's fault), else 0.  Synchronises the stream before returning.
hipError_t build_unitigs(UnitigBuffers* B, const UnitigNodes& nd, const EdgeResult& ed, hipStream_t s, UnitigResult* out, int* broken);
