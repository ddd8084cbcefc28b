// superbubbles.h — interface between the simplification stage (simplify.hip) and the SUPERBUBBLES step's translation unit (superbubbles.hip).  Definition:
// include/mdbg_hip.h (mdbg_graph_simplify, MDBG_SIMPLIFY_SUPERBUBBLES).  Included by those two translation units only (it shows the compaction's buffers, unitigs_priv.h).
#pragma once
#include "simplify.h"
#include "unitigs_priv.h"

// The step on the list `ul` of the last compaction in B, whose sorted arcs, settled ranking, flag and uid it reads; uhead / utail: the first and the last vertex of
// every unitig of that list (simplify.hip's ends_kernel, queued before).  Queues two memsets and four kernels and waits for nothing: rem[u] <- 1 for every unitig
// the step removes (0 for the others), ctr[0] <- their number; *defect_flag <- where the device sets a nonzero word if it meets a vertex outside the arrays or a
// best chain that does not end at its source (the caller reads it back with its counters, in the wait every removing step has).
hipError_t superbubbles_run(UnitigBuffers* B, const UnitigResult& ul, u32 n2x, const u32* uhead, const u32* utail, u32 max_nodes, u64 max_bases, u8* rem, u32* ctr,
                            hipStream_t s, const u32** defect_flag);
