// simplify.hip — tip clipping, simple-bubble popping, small-component removal and the pruning of edges no read crosses, on the unitig graph, on the GPU (gfx950).
// It reads the arrays of the compaction stage (unitigs.hip; shown by unitigs_priv.h: sorted arcs, settled ranking, unitig numbers, lengths, abundance sums, the
// records' vertices and unitig edge positions) and calls that compaction again under a node mask and, once an EDGES step has removed a record, a record mask.
//
// The rules are the ones written out in include/mdbg_hip.h (mdbg_graph_simplify): this project's own order-free definition in the spirit of
// `gfatools asm -t N,L -b L`, NOT gfatools' in-place passes.  A step decides against the graph as it is when the step starts, so every kernel below reads
// one compaction and only the last one writes the mask.
//
// Adjacency comes from the ONE sorted arc array of the compaction (source, target): the out-arcs of x are the run with source x (binary search), and because
// the arc set is closed under mirroring the in-neighbours of w are the complements of the out-targets of comp(w).  No second sort, no degree atomics.
//
//   ends_kernel          kept head -> first and last vertex of its unitig
//   tip_cand_kernel      small unitig with exactly one dead end -> its attached vertex x (att[unitig], owner[x])
//   tip_decide_kernel    candidate u is removed iff every target of x has another in-neighbour that is no candidate's attached vertex or a better candidate's
//   bubble_key_kernel    small unitig with one way in (p) and one way out (q), p / q not on it, q != comp(p) -> key min((p,q), (comp q, comp p)); rocPRIM sorts (key, unitig)
//   bubble_decide_kernel first entry of every run of equal keys: the best member stays, the others are removed
//   comp_decide_kernel   unitig of a small component (components.hip: nodes, bases and circular summed per component) -> removed
//   scatter_kernel       vertices of removed unitigs -> alive[row] = 0; counts the nodes
//
// MDBG_SIMPLIFY_EDGES removes edge records, not nodes: the junction stage (junctions.hip) counts the reads that cross each unitig edge record of the current
// list, and two kernels over the node-level records of the last compaction (eu / ev: their vertices, ekeep / epos: their unitig record) decide:
//   edge_mark_kernel     kept record whose unitig record has support >= min_support -> strong[eu] = strong[comp(ev)] = 1 (plain stores of one value)
//   edge_decide_kernel   kept weak record with strong[eu] and strong[comp(ev)] -> edge_alive[e] = 0; counts the records
// The record mask is closed under mirroring and duplication because equal junction keys carry equal supports; the next compaction takes it beside the node mask.
//
// MDBG_SIMPLIFY_REPEATS removes nothing: the transit stage (transits.hip) says which unitigs of the current list the reads resolve, and repeats.hip appends the
// copies to the node columns, the masks and the edge records; the next compaction takes the larger graph as any other, and the schedule goes on with it.  The
// list's node[] names the originals: one kernel at the end of the schedule (repeats_report_originals).
// MDBG_SIMPLIFY_NESTED is the same branch.  Once the schedule has made copies it hands the transit stage the origin map {X, copies so far, origin[]}, so that the
// windows are placed on a list that holds copies (placement.hip), and the step itself the earlier result, so that it grows into fresh blocks (repeats.hip).
//
// MDBG_SIMPLIFY_SUPERBUBBLES has a translation unit of its own (superbubbles.hip): it reads uhead / utail of ends_kernel and the sorted arcs, writes rem[] and the unitig
// counter, and shares scatter_kernel and the one wait with the other removing kinds; its defect word travels in that wait as a component step's does.
//
// Host round trips per step: those of one compaction (unitigs.hip) plus ONE for the two removal counters, which size the next compaction's checks; an EDGES step
// waits once for its junction stage and once for its counter; a REPEATS step once for its transit stage and, if something resolves, once for the totals that size
// the copies and once for its defect flag; a NESTED step waits as a REPEATS step does, with or without copies in the graph (the placement's extra launches ride in the transit
// stage's wait).  A step that removes nothing is followed by no compaction: the next step decides on the same arrays.
#include <cstring>

#include "repeats.h"
#include "simplify.h"
#include "superbubbles.h"
#include "unitigs_priv.h"

namespace {

struct SimpArgs {
    u32 n2x; u64 U, n_arcs; const u64* sk;
    const u32* P; const u32* prv; const u32* flag; const u32* uid; const u8* cyc;
    const u64* offsets; const u64* length; const u64* kc; const u8* circ;
    u32 max_nodes; u64 max_bases;
    u32* uhead; u32* utail; u32* att; u32* owner; u8* rem; u64* bkey; u32* bval; const u64* skey; const u32* sval; u32* ctr; u8* alive;
};

__device__ inline u64 arcs_from(const SimpArgs& a, u32 x) {      // first sorted arc whose source is >= x
    const u64 key = (u64)x << 32;
    u64 lo = 0, hi = a.n_arcs;
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.sk[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// number of distinct targets of x, counted up to 2; *only <- the first one
__device__ inline u32 out_degree2(const SimpArgs& a, u32 x, u32* only) {
    u32 n = 0; u64 last = 0;
    for (u64 i = arcs_from(a, x); i < a.n_arcs && (u32)(a.sk[i] >> 32) == x && n < 2; ++i) {
        const u64 k = a.sk[i];
        if (n && k == last) continue;
        if (!n) *only = (u32)k;
        last = k; ++n;
    }
    return n;
}
__device__ inline bool is_small(const SimpArgs& a, u64 u) {
    return !a.circ[u] && (a.max_nodes == 0 || a.offsets[u + 1] - a.offsets[u] <= a.max_nodes) && (a.max_bases == 0 || a.length[u] <= a.max_bases);
}
// a ranks above b: mean abundance kc / entries compared exactly (128-bit cross products), then the longer, then the smaller number
__device__ inline bool beats(const SimpArgs& a, u32 x, u32 y) {
    const u64 nx = a.offsets[x + 1] - a.offsets[x], ny = a.offsets[y + 1] - a.offsets[y];
    const u64 lx = a.kc[x] * ny, hx = __umul64hi(a.kc[x], ny), ly = a.kc[y] * nx, hy = __umul64hi(a.kc[y], nx);
    if (hx != hy) return hx > hy;
    if (lx != ly) return lx > ly;
    if (a.length[x] != a.length[y]) return a.length[x] > a.length[y];
    return x < y;
}
__device__ inline u32 unitig_at(const SimpArgs& a, u32 v) {      // the unitig the node of v lies on
    u32 h = a.P[v] & ~TERM;
    if (!a.flag[h]) h = a.P[v ^ 1] & ~TERM;
    return a.uid[h];
}

__global__ __launch_bounds__(256) void ends_kernel(SimpArgs a) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n2x || (a.P[v] & ~TERM) != v || !a.flag[v]) return;
    const u32 u = a.uid[v];
    if (u >= a.U) return;
    a.uhead[u] = v;
    a.utail[u] = (a.cyc && a.cyc[v]) ? a.prv[v] : ((a.P[v ^ 1] & ~TERM) ^ 1);
}

__global__ __launch_bounds__(256) void tip_cand_kernel(SimpArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    u32 x = NONE;
    if (is_small(a, u)) {
        const u32 h = a.uhead[u], t = a.utail[u];
        u32 dummy;
        const bool fwd = out_degree2(a, h ^ 1, &dummy) == 0;      // nothing enters the first vertex  (in-arcs of h = out-arcs of comp(h))
        const bool rev = out_degree2(a, t, &dummy) == 0;          // nothing enters comp(last)
        if (fwd != rev) x = fwd ? t : (h ^ 1);
    }
    a.att[u] = x;
    if (x != NONE && x < a.n2x) a.owner[x] = (u32)u;              // an attached vertex belongs to one unitig only
}

__global__ __launch_bounds__(256) void tip_decide_kernel(SimpArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool gone = false;
    if (u < a.U) {
        const u32 x = a.att[u];
        if (x != NONE) {
            gone = true;                                          // (x has an out-arc: its other end is the dead one)
            for (u64 i = arcs_from(a, x); gone && i < a.n_arcs && (u32)(a.sk[i] >> 32) == x; ++i) {
                const u32 w = (u32)a.sk[i];
                bool other = false;
                for (u64 j = arcs_from(a, w ^ 1); !other && j < a.n_arcs && (u32)(a.sk[j] >> 32) == (w ^ 1); ++j) {
                    const u32 y = (u32)a.sk[j] ^ 1;               // an in-neighbour of w
                    if (y == x || y >= a.n2x) continue;
                    const u32 c = a.owner[y];
                    other = c == NONE || beats(a, c, (u32)u);
                }
                gone = other;
            }
        }
        a.rem[u] = gone ? 1 : 0;
    }
    count_to(a.ctr, gone);
}

__global__ __launch_bounds__(256) void bubble_key_kernel(SimpArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    u64 key = ~0ull;
    if (is_small(a, u)) {
        const u32 h = a.uhead[u], t = a.utail[u];
        u32 y = 0, q = 0;
        if (out_degree2(a, h ^ 1, &y) == 1 && out_degree2(a, t, &q) == 1 && y < a.n2x && q < a.n2x) {
            const u32 p = y ^ 1;
            if (q != (p ^ 1) && unitig_at(a, p) != u && unitig_at(a, q) != u) {
                const u64 k1 = ((u64)p << 32) | q, k2 = ((u64)(q ^ 1) << 32) | (p ^ 1);
                key = k1 < k2 ? k1 : k2;
            }
        }
    }
    a.bkey[u] = key; a.bval[u] = (u32)u; a.rem[u] = 0;
}

__global__ __launch_bounds__(256) void bubble_decide_kernel(SimpArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 gone = 0;
    if (i < a.U) {
        const u64 key = a.skey[i];
        if (key != ~0ull && (i == 0 || a.skey[i - 1] != key)) {
            u32 best = a.sval[i]; u64 j = i + 1;
            for (; j < a.U && a.skey[j] == key; ++j) { const u32 c = a.sval[j]; if (c < a.U && beats(a, c, best)) best = c; }
            if (j > i + 1)
                for (u64 m = i; m < j; ++m) { const u32 c = a.sval[m]; if (c != best && c < a.U) { a.rem[c] = 1; ++gone; } }
        }
    }
    if (gone) atomicAdd(a.ctr, gone);
}

// MDBG_SIMPLIFY_COMPONENTS: the limits apply to the component's sums, not to the unitig
__global__ __launch_bounds__(256) void comp_decide_kernel(SimpArgs a, const u32* __restrict__ component, const u64* __restrict__ c_nodes, const u64* __restrict__ c_bases,
                                                          const u8* __restrict__ c_circ) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool gone = false;
    if (u < a.U) {
        const u32 c = component[u];
        gone = c < a.U && !c_circ[c] && (a.max_nodes == 0 || c_nodes[c] <= a.max_nodes) && (a.max_bases == 0 || c_bases[c] <= a.max_bases);
        a.rem[u] = gone ? 1 : 0;
    }
    count_to(a.ctr, gone);
}

__global__ __launch_bounds__(256) void scatter_kernel(SimpArgs a) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    bool gone = false;
    if (v < a.n2x) {
        const u32 h = a.P[v] & ~TERM;
        if (a.flag[h]) { const u32 u = a.uid[h]; gone = u < a.U && a.rem[u]; }
        if (gone) a.alive[v >> 1] = 0;
    }
    count_to(a.ctr + 1, gone);
}

// MDBG_SIMPLIFY_EDGES.  Node-level record e of the last compaction: vertices eu[e] -> ev[e] (NONE: an end or the record was removed before), ekeep[e] = it is a
// unitig edge record, the one at epos[e] of the current list (an interior link has none and is never touched)
struct EdgeArgs {
    u64 n_edges, n_records; u32 n2x, min_support;
    const u32* eu; const u32* ev; const u32* ekeep; const u32* epos; const u64* support;
    u8* strong; u8* edge_alive; u32* ctr;
};
__device__ inline bool edge_record(const EdgeArgs& a, u64 e, u32* x, u32* cy, bool* is_strong) {      // false: no unitig edge record (or one outside the arrays: never indexed)
    if (e >= a.n_edges || !a.ekeep[e]) return false;
    const u32 u = a.eu[e], v = a.ev[e], r = a.epos[e];
    if (u >= a.n2x || v >= a.n2x || r >= a.n_records) return false;
    *x = u; *cy = v ^ 1; *is_strong = a.support[r] >= a.min_support;
    return true;
}
__global__ __launch_bounds__(256) void edge_mark_kernel(EdgeArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 x, cy; bool is_strong;
    if (edge_record(a, e, &x, &cy, &is_strong) && is_strong) { a.strong[x] = 1; a.strong[cy] = 1; }      // reads leave x here, and comp(y) by the mirror
}
__global__ __launch_bounds__(256) void edge_decide_kernel(EdgeArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 x, cy; bool is_strong;
    const bool gone = edge_record(a, e, &x, &cy, &is_strong) && !is_strong && a.strong[x] && a.strong[cy];
    if (gone) a.edge_alive[e] = 0;
    count_to(a.ctr, gone);
}

}  // namespace

hipError_t simplify_unitigs(UnitigBuffers* B, ComponentBuffers* CB, const SimplifySupport* sup, const UnitigNodes& nd0, const EdgeResult& ed0, const mdbg_simplify_step* steps, uint32_t n_steps,
                     hipStream_t s, UnitigResult* out, uint64_t* unitigs_removed, uint64_t* nodes_removed, uint64_t* edges_removed, SimplifyInfo* info, int* broken) {
    memset(info, 0, sizeof *info);
    for (uint32_t k = 0; k < n_steps; ++k) edges_removed[k] = 0;
    if (n_steps == 0 || nd0.n == 0) {                         // the empty schedule IS the unitig call
        const hipError_t rc = build_unitigs(B, nd0, ed0, s, out, broken);
        if (rc == hipSuccess && !*broken && nd0.n) { info->n_compactions = 1; info->n_rounds_total = out->n_rounds; info->n_syncs = out->n_rounds + 3 + (ed0.n ? 1 : 0); }
        return rc;
    }
    UnitigNodes nd = nd0; EdgeResult ed = ed0;               // a REPEATS step replaces both by the graph with the copies
    u64 n = nd.n;
    *broken = 0;
    if (n >= (1ull << 30)) return defect(broken);
    u32 n2x = (u32)(2 * n);
    RepeatsResult rr; memset(&rr, 0, sizeof rr);
    GHIP(B->alive.ensure(n));
    GHIP(hipMemsetAsync(B->alive.p, 1, n, s));
    u8* alive = B->alive.as<u8>();
    u64 n_alive = n;
    const u8* edge_alive = nullptr;                           // null until an EDGES step removes a record: a schedule without one compacts as it always did
    bool stale = true;                                        // the arrays of the last compaction no longer describe the surviving graph
    auto compact = [&]() -> hipError_t {
        if (n_alive == 0) { memset(out, 0, sizeof *out); stale = false; return hipSuccess; }      // a step removed all that was left: the empty list, nothing to launch
        GHIP(build_unitigs_masked(B, nd, ed, alive, n_alive, edge_alive, s, out, broken));
        if (*broken) return hipSuccess;
        ++info->n_compactions; info->n_rounds_total += out->n_rounds; info->n_syncs += out->n_rounds + 3 + (ed.n ? 1 : 0);
        stale = false;
        return hipSuccess;
    };
    for (uint32_t k = 0; k < n_steps; ++k) {
        unitigs_removed[k] = 0; nodes_removed[k] = 0;
        if (stale) { GHIP(compact()); if (*broken) return hipSuccess; }
        const u64 U = out->n_unitigs;
        if (U == 0) continue;
        if (steps[k].kind == MDBG_SIMPLIFY_EDGES) {
            if (!sup) return hipErrorInvalidValue;
            const u64 E = ed.n, UE = out->edges.n;
            if (!sup->has_reads || E == 0 || UE == 0) continue;      // nothing is strong, or there is no record: the step removes nothing
            if (!edge_alive) { GHIP(B->edge_alive.ensure(E)); GHIP(hipMemsetAsync(B->edge_alive.p, 1, E, s)); }      // (not handed to a compaction before a record goes)
            GHIP(B->strong.ensure(n2x));
            JunctionResult jr;
            GHIP(junctions_run(sup->jb, sup->pb, *out, sup->index, sup->n_rows, sup->range, sup->placer, s, &jr));
            ++info->n_syncs; info->junction_ms += jr.ms;
            if (jr.defect) { info->junction_defect = jr.defect; return defect(broken); }
            if (jr.n_records != UE) return defect(broken);
            u32* d_ctr = B->ctr.as<u32>();                    // (the compaction is over: its round counters are free)
            GHIP(hipMemsetAsync(d_ctr, 0, 4, s));
            GHIP(hipMemsetAsync(B->strong.p, 0, n2x, s));
            EdgeArgs ea; memset(&ea, 0, sizeof ea);
            ea.n_edges = E; ea.n_records = UE; ea.n2x = n2x; ea.min_support = steps[k].max_nodes;
            ea.eu = B->eu.as<u32>(); ea.ev = B->ev.as<u32>(); ea.ekeep = B->ekeep.as<u32>(); ea.epos = B->epos.as<u32>(); ea.support = jr.support;
            ea.strong = B->strong.as<u8>(); ea.edge_alive = B->edge_alive.as<u8>(); ea.ctr = d_ctr;
            hipLaunchKernelGGL(edge_mark_kernel, dim3(grid_for(E)), dim3(256), 0, s, ea);
            hipLaunchKernelGGL(edge_decide_kernel, dim3(grid_for(E)), dim3(256), 0, s, ea);
            u32 gone = 0;
            GHIP(hipMemcpyAsync(&gone, d_ctr, 4, hipMemcpyDeviceToHost, s));
            GHIP(hipStreamSynchronize(s));
            ++info->n_syncs;
            if (gone > UE) return defect(broken);
            edges_removed[k] = gone;
            if (gone) { edge_alive = B->edge_alive.as<u8>(); stale = true; }
            continue;
        }
        if (steps[k].kind == MDBG_SIMPLIFY_REPEATS || steps[k].kind == MDBG_SIMPLIFY_NESTED) {
            if (!sup || !sup->tb) return hipErrorInvalidValue;
            const bool holds_copies = rr.total_copies != 0;      // (the validation admits a NESTED step only: REPEATS means "the graph holds no copies")
            if (holds_copies && steps[k].kind != MDBG_SIMPLIFY_NESTED) return hipErrorInvalidValue;
            if (!sup->has_reads || ed.n == 0 || out->edges.n == 0) continue;      // nothing resolves without reads, and a repeat has records
            TransitResult tr;
            if (holds_copies) GHIP(transits_run(sup->tb, sup->pb, *out, sup->index, sup->n_rows, sup->range, steps[k].max_nodes, sup->placer, s, &tr, OriginMap{rr.first_copy_index, rr.total_copies, rr.origin}));
            else GHIP(transits_run(sup->tb, sup->pb, *out, sup->index, sup->n_rows, sup->range, steps[k].max_nodes, sup->placer, s, &tr));
            ++info->n_syncs; info->transit_ms += tr.ms;
            info->ambiguous += tr.ambiguous; info->resolved += tr.resolved; info->conflicts += tr.conflicts; info->unanchored += tr.unanchored;
            if (tr.defect) { info->transit_defect = tr.defect; return defect(broken); }
            if (tr.n_unitigs != U) return defect(broken);
            if (tr.n_resolved == 0 || tr.n_transits == 0) continue;
            RepeatsResult step;
            GHIP(repeats_run(B, tr, steps[k].max_nodes, *out, nd, ed, alive, edge_alive, nd0.index + (nd0.n - 1), holds_copies ? &rr : nullptr, s, &step));
            info->n_syncs += step.too_large ? 1 : 2;
            if (step.too_large) { info->repeats_too_large = true; return defect(broken); }
            if (step.defect) { info->repeats_defect = step.defect; return defect(broken); }
            if (step.copies == 0) return defect(broken);      // a resolved unitig has two entrances and an entry
            rr = step;
            nd = rr.nd; ed = rr.ed; alive = rr.alive; edge_alive = rr.edge_alive;
            n = nd.n; n2x = (u32)(2 * n); n_alive += rr.copies; info->copies = rr.total_copies;
            stale = true;
            continue;
        }
        GHIP(B->uhead.ensure(n * 4)); GHIP(B->utail.ensure(n * 4)); GHIP(B->att.ensure(n * 4)); GHIP(B->rem.ensure(n)); GHIP(B->owner.ensure((size_t)n2x * 4));
        u32* d_ctr = B->ctr.as<u32>();                        // (the compaction is over: its round counters are free)
        GHIP(hipMemsetAsync(d_ctr, 0, 8, s));
        SimpArgs a; memset(&a, 0, sizeof a);
        a.n2x = n2x; a.U = U; a.n_arcs = B->n_arcs; a.sk = B->skeys.as<u64>(); a.P = B->Pfin; a.prv = B->prv.as<u32>(); a.flag = B->flag.as<u32>(); a.uid = B->uid.as<u32>(); a.cyc = B->cycfin;
        a.offsets = out->offsets; a.length = out->length; a.kc = out->kc_sum; a.circ = out->circular; a.max_nodes = steps[k].max_nodes; a.max_bases = steps[k].max_bases;
        a.uhead = B->uhead.as<u32>(); a.utail = B->utail.as<u32>(); a.att = B->att.as<u32>(); a.owner = B->owner.as<u32>(); a.rem = B->rem.as<u8>(); a.ctr = d_ctr; a.alive = alive;
        const unsigned gu = grid_for(U), gv = grid_for(n2x);
        const u32* d_cstatus = nullptr;                       // a component or superbubble step: where its stage reports a defect
        if (steps[k].kind == MDBG_SIMPLIFY_COMPONENTS) {
            if (!CB) return hipErrorInvalidValue;
            ComponentResult cr;
            GHIP(queue_components(CB, *out, s, &cr));
            hipLaunchKernelGGL(comp_decide_kernel, dim3(gu), dim3(256), 0, s, a, cr.component, cr.nodes, cr.bases, cr.circular);
            d_cstatus = cr.status;
        } else {
            hipLaunchKernelGGL(ends_kernel, dim3(gv), dim3(256), 0, s, a);
            if (steps[k].kind == MDBG_SIMPLIFY_TIPS) {
                GHIP(hipMemsetAsync(B->owner.p, 0xFF, (size_t)n2x * 4, s));
                hipLaunchKernelGGL(tip_cand_kernel, dim3(gu), dim3(256), 0, s, a);
                hipLaunchKernelGGL(tip_decide_kernel, dim3(gu), dim3(256), 0, s, a);
            } else if (steps[k].kind == MDBG_SIMPLIFY_SUPERBUBBLES) {
                GHIP(superbubbles_run(B, *out, n2x, a.uhead, a.utail, a.max_nodes, a.max_bases, a.rem, d_ctr, s, &d_cstatus));      // (superbubbles.hip: rem[] and the unitig counter)
            } else {
                GHIP(B->bkey.ensure(n * 8)); GHIP(B->bkey2.ensure(n * 8)); GHIP(B->bval.ensure(n * 4)); GHIP(B->bval2.ensure(n * 4));
                a.bkey = B->bkey.as<u64>(); a.bval = B->bval.as<u32>(); a.skey = B->bkey2.as<u64>(); a.sval = B->bval2.as<u32>();
                hipLaunchKernelGGL(bubble_key_kernel, dim3(gu), dim3(256), 0, s, a);
                GHIP(sort_pairs(B->tmp, a.bkey, B->bkey2.as<u64>(), a.bval, B->bval2.as<u32>(), (size_t)U, 0, 64, s));
                hipLaunchKernelGGL(bubble_decide_kernel, dim3(gu), dim3(256), 0, s, a);
            }
        }
        hipLaunchKernelGGL(scatter_kernel, dim3(gv), dim3(256), 0, s, a);
        u32 got[2], cdefect = 0;
        GHIP(hipMemcpyAsync(got, d_ctr, 8, hipMemcpyDeviceToHost, s));
        if (d_cstatus) GHIP(hipMemcpyAsync(&cdefect, d_cstatus, 4, hipMemcpyDeviceToHost, s));      // (the same wait: a component step costs no synchronisation of its own)
        GHIP(hipStreamSynchronize(s));
        ++info->n_syncs;
        if (cdefect) return defect(broken);
        if (got[1] > n_alive || got[0] > U || (got[0] == 0) != (got[1] == 0)) return defect(broken);
        unitigs_removed[k] = got[0]; nodes_removed[k] = got[1];
        n_alive -= got[1];
        stale = got[1] != 0;
    }
    if (stale) { GHIP(compact()); if (*broken) return hipSuccess; }
    if (rr.total_copies) { GHIP(repeats_report_originals(B, *out, rr, s)); GHIP(hipStreamSynchronize(s)); ++info->n_syncs; }
    return hipGetLastError();
}
