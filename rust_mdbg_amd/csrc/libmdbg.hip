// libmdbg.hip — main translation unit of libmdbg_hip.so (gfx950); the graph stages (edges.hip and the others over graph_common.h: rocPRIM sorts / scans) are compiled separately.
// The device files in dependency order — sketch, small helpers, counting table, its counting pre-filter, owners (multi-GPU partition), finalize, the window placing of the read paths, synthetic reads, routing — then the host side.
#include "sketch.hip"
#include "dev_util.hip"
#include "table.hip"
#include "prefilter.hip"
#include "owner.hip"
#include "finalize.hip"
#include "place_windows.hip"
#include "synth.hip"
#include "route.hip"
#include "api.inc"
#include "dist_api.inc"
