// unitigs_priv.h — what the compaction (unitigs.hip) shows the simplification stage (simplify.hip, repeats.hip, superbubbles.hip): its buffers, its vertex codes and the masked compaction.
// Included by those four translation units only.
#pragma once
#include "graph_common.h"
#include "unitigs.h"

namespace {

constexpr u32 NONE = 0xFFFFFFFFu;      // no successor / no link
constexpr u32 TERM = 0x80000000u;      // on a jump pointer: it names the chain head, the distance is final (vertices are < 2^31)

__device__ inline void count_to(u32* ctr, bool pred) { if (pred) atomicAdd(ctr, 1u); }      // (the compiler folds a wave's adds into one atomic of the active-lane count)

inline hipError_t defect(int* broken) { *broken = 1; return hipSuccess; }      // the `broken` outcome of unitigs.h

}  // namespace

struct UnitigBuffers {
    Buf keys, skeys, eu, ev, succ, nxt, prv, P[2], D[2], M[2], cyc, flag, hlen, uid, hoff, ctr, tmp;
    Buf offsets, node, ori, src_read, src_begin, len, rc, dst, ent_u, pl64, ab64, gs, ga, length, kc, circ;
    Buf ekeep, epos, un1, un2, uov, uo1, uo2;
    // what the last build_unitigs left for simplify.hip: the settled ranking (one of P[] / D[]), the cycle marks (or null) and the number of sorted arcs in skeys
    const u32* Pfin = nullptr; const u32* Dfin = nullptr; const u8* cycfin = nullptr; u64 n_arcs = 0;
    Buf alive, uhead, utail, att, owner, rem, bkey, bkey2, bval, bval2;      // simplify.hip
    Buf edge_alive, strong;                                                  // simplify.hip, EDGES steps: the record mask, the vertices with a strong exit
    // repeats.hip, the REPEATS step: its temporaries (per transit row, per unitig, per record), then the node columns, masks and edge records extended by the copies
    Buf x_strong, x_rank, x_rows, x_rowbase, x_ecnt, x_ebase, x_ctr;
    Buf x_index, x_abund, x_shift, x_sread, x_sstart, x_send, x_rev, x_alive, x_origin, x_n1, x_o1, x_n2, x_o2, x_ov, x_ealive;
    Buf sb_cand, sb_app, sb_J, sb_ctr;      // superbubbles.hip, the SUPERBUBBLES step: candidate sources, canonical fitting sources, the interiors' unitigs, its counters
};

// build_unitigs restricted by `alive` (device, one byte per row of the node table; null = every node) to the surviving nodes and the arcs between them; n_alive = how many;
// and by `edge_alive` (device, one byte per record of `ed`; null = every record) to the arcs of the surviving records: a record with edge_alive[e] == 0 is treated
// exactly as a record with a removed end.  The mask must be closed under mirroring and duplication (a record, its mirror record and their copies fall together).
// (not part of the library's surface: hidden, as it was while it was static)
__attribute__((visibility("hidden"))) hipError_t build_unitigs_masked(UnitigBuffers* B, const UnitigNodes& nd, const EdgeResult& ed, const u8* alive, u64 n_alive, const u8* edge_alive, hipStream_t s, UnitigResult* out, int* broken);
