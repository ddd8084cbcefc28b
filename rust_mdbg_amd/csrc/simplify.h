// simplify.h — interface between the C ABI (api.inc) and the simplification stage (simplify.hip).
#pragma once
#include "../../include/mdbg_hip.h"
#include "components.h"
#include "unitigs.h"

struct SimplifyInfo { uint32_t n_compactions, n_rounds_total, n_syncs; };      // compactions run, their jumping rounds, host synchronisations of the whole call
// Runs the schedule on the node table and edge list (mdbg_graph_simplify, include/mdbg_hip.h) and leaves the unitig list of the surviving graph in *out, in
// the same buffers as build_unitigs (valid until the next call of either).  unitigs_removed / nodes_removed: n_steps host entries.  Return value and *broken as build_unitigs.
// CB: the component stage's buffers, used by MDBG_SIMPLIFY_COMPONENTS steps (may be null when the schedule has none).
hipError_t simplify_unitigs(UnitigBuffers* B, ComponentBuffers* CB, const UnitigNodes& nd, const EdgeResult& ed, const mdbg_simplify_step* steps, uint32_t n_steps, hipStream_t s, UnitigResult* out,
                     uint64_t* unitigs_removed, uint64_t* nodes_removed, SimplifyInfo* info, int* broken);
