// components.h — interface between the C ABI (api.inc), the simplification stage (simplify.hip) and the connected-components stage (components.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unitigs.h"

struct ComponentBuffers;           // scratch + results, owned by the context (opaque here)
ComponentBuffers* component_buffers_create();
void component_buffers_destroy(ComponentBuffers*);

struct ComponentResult {           // device pointers into ComponentBuffers, valid until the next call; the per-component arrays have room for n_unitigs entries
    uint64_t n_unitigs, n_components;
    const uint32_t* component;     // n_unitigs
    const uint32_t* first_unitig; const uint32_t* unitigs; const uint64_t* nodes; const uint64_t* bases; const uint64_t* kc_sum; const uint8_t* circular;      // n_components
    const uint32_t* status;        // two words: [0] != 0: a find or a retry ran into its bound (a defect), [1] = the number of components
};
// Components of the unitig list `ul` (mdbg_graph_components, include/mdbg_hip.h) by a fixed number of launches, whatever the input.
// queue_components only queues them on the stream: out->n_components stays 0 and out->status says the rest once the stream has passed
// (simplify.hip reads it with its step's counters).  build_components also waits ONCE, for status: *broken <- 1 (with hipSuccess) on a defect, as build_unitigs.
hipError_t queue_components(ComponentBuffers* B, const UnitigResult& ul, hipStream_t s, ComponentResult* out);
hipError_t build_components(ComponentBuffers* B, const UnitigResult& ul, hipStream_t s, ComponentResult* out, int* broken);
