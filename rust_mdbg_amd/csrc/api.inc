// api.inc — context management and the C ABI of include/mdbg_hip.h (host code; included by libmdbg.hip after the device files, sketch.hip .. route.hip, so that
// it sees their launchers and argument structs).  Its parts, in the order they depend on each other:
#include <algorithm>
#include <cstdio>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mdbg_hip.h"
#include "../../include/mdbg_align.h"
#include "../../include/mdbg_chain.h"
#include "edges.h"
#include "unitigs.h"
#include "simplify.h"
#include "components.h"
#include "contigs.h"
#include "node_seqs.h"
#include "placement.h"
#include "read_paths.h"
#include "junctions.h"
#include "transits.h"
#include "alignments.h"
#include "chains.h"

#include "blocks.inc"
#include "results.inc"      // the derived graph results and which of them are current
#include "context.inc"
#include "store.inc"
#include "prefilter_api.inc"   // the counting pre-filter in front of the table (MDBG_FLAG_PREFILTER)
#include "ingest_api.inc"
extern "C" {                   // entry points and their static helpers only from here on
#include "finalize_api.inc"
#include "graph_api.inc"      // edges, unitigs, simplification, contigs, node sequences, read paths, junction support, transits
#include "import_api.inc"
}
#include "route_api.inc"      // multi-GPU routing
