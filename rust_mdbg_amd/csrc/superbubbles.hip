// superbubbles.hip — the SUPERBUBBLES step of a simplify schedule: pop bubbles whose inside branches, on the GPU (gfx950).  Definition: include/mdbg_hip.h
// (mdbg_graph_simplify, MDBG_SIMPLIFY_SUPERBUBBLES).  Input, all on the device: the ONE sorted arc array of the last compaction (source, target), the settled ranking
// with flag / uid (node vertex -> unitig), uhead / utail per unitig, and the list's offsets, length, kc_sum and circular.
//
// Coordinates.  An ORIENTED UNITIG is ov = 2 * u + strand.  It is entered at entry(ov) = uhead[u] (strand 0) or comp(utail[u]) and left at exit(ov) = utail[u] or
// comp(uhead[u]); its out-arcs are the run of the sorted arcs with source exit(ov), and every target of such a run is the entry of an oriented unitig.  Because the
// arc set is closed under mirroring, the in-degree of the vertex entered at w is the number of distinct targets of the run with source comp(w).
//
//   sb_cand_kernel    one thread per oriented unitig: two distinct out-targets -> appended to the candidate list (the order of the list decides nothing)
//   sb_find_kernel    one WAVE per candidate source s, a fixed grid striding over the list.  The visited set lives in the wave: slot i (lane i & 63, register i >> 6)
//                     holds visited vertex i: its oriented unitig, the in-arcs not yet seen, the best in-neighbour so far (slot and unitig) and val as the number of
//                     the unitig whose mean it is.  "Is w visited" is a compare and a ballot, appending takes the next slot, slot 66 fails the source (65 = 64 interior
//                     vertices and the sink).  Kahn's order: a vertex is expanded when all its in-arcs were seen, the lanes read its run together, each distinct
//                     target is looked up or appended, and the source stops as soon as one vertex is ready, none waits and all others are expanded: that one is t.
//                     A fitting bubble stores 1 into J[u] for the unitigs of its interior, and its source is appended to the list of canonical readings if u(s) < u(t)
//   sb_decide_kernel  one wave per canonical fitting source: J[u(s)] or J[u(t)] set -> not applied.  Else the same traversal again (it is a function of the arrays
//                     alone, so it gives the same slots), the best chain from t marks the kept slots, and every other interior unitig gets rem = 1
//   sb_count_kernel   one thread per unitig: the removal counter
//
// Nothing is kept per source but its place in a list: the temporaries are 17 bytes per unitig (two lists of 4 bytes per oriented unitig, one byte of J).  Every loop is bounded by the cap or by a run of
// the arc array: an expansion reads its source's run in pieces of 64 and fails on the 66th vertex, an in-degree is counted up to 66, at most 65 vertices are expanded.
// Positions and decisions come from integers only (the means by 128-bit cross products); the two atomics append to lists whose order is never read.
#include <cstring>

#include "../../include/mdbg_hip.h"
#include "superbubbles.h"

namespace {

constexpr u32 MAXU = MDBG_SUPERBUBBLE_MAX_UNITIGS;      // interior vertices
constexpr u32 CAP = MAXU + 1;                           // slots: the interior and the sink
constexpr u32 SLOT_S = 0xFFFFu;                         // "the source" where a slot is named
static_assert(CAP <= 128, "two slots per lane");
enum : u32 { SB_NO = 0, SB_YES = 1, SB_DEFECT = 2 };

struct SbArgs {
    u32 n2x; u64 U, n_arcs; const u64* sk;
    const u32* P; const u32* flag; const u32* uid; const u32* uhead; const u32* utail;
    const u64* offsets; const u64* length; const u64* kc; const u8* circ;
    u32 max_nodes; u64 max_bases;
    u32* cand; u32* app; u8* J; u32* sctr;              // sctr: [0] candidates, [1] canonical fitting sources, [2] the defect word
    u8* rem; u32* ctr;
};

__device__ inline u64 lower_bound(const SbArgs& a, u64 key) {      // first sorted arc >= key
    u64 lo = 0, hi = a.n_arcs;
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.sk[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ inline u32 entry_of(const SbArgs& a, u32 ov) { return (ov & 1) ? a.utail[ov >> 1] ^ 1u : a.uhead[ov >> 1]; }
__device__ inline u32 exit_of(const SbArgs& a, u32 ov) { return (ov & 1) ? a.uhead[ov >> 1] ^ 1u : a.utail[ov >> 1]; }
// node vertex w -> the oriented unitig entered there; false: w lies outside the arrays or is no unitig's end (a defect: nothing is indexed with it)
__device__ inline bool oriented_at(const SbArgs& a, u32 w, u32* ov) {
    if (w >= a.n2x) return false;
    u32 h = a.P[w] & ~TERM;
    if (h < a.n2x && !a.flag[h]) h = a.P[w ^ 1u] & ~TERM;
    if (h >= a.n2x || !a.flag[h]) return false;
    const u32 u = a.uid[h];
    if (u >= a.U) return false;
    if (w == a.uhead[u]) *ov = 2 * u;
    else if (w == (a.utail[u] ^ 1u)) *ov = 2 * u + 1;
    else return false;
    return true;
}
__device__ inline u64 entries(const SbArgs& a, u32 u) { return a.offsets[u + 1] - a.offsets[u]; }
// mean(x) > mean(y), exactly
__device__ inline bool mean_above(const SbArgs& a, u32 x, u32 y) {
    const u64 nx = entries(a, x), ny = entries(a, y);
    const u64 lx = a.kc[x] * ny, hx = __umul64hi(a.kc[x], ny), ly = a.kc[y] * nx, hy = __umul64hi(a.kc[y], nx);
    return hx != hy ? hx > hy : lx > ly;
}
// val is named by the unitig whose mean it is; NONE = val(s) = +infinity
__device__ inline bool val_above(const SbArgs& a, u32 x, u32 y) {
    if (x == NONE || y == NONE) return x == NONE && y != NONE;
    return mean_above(a, x, y);
}
// the total order of the other kinds: mean, then the longer, then the smaller number
__device__ inline bool beats(const SbArgs& a, u32 x, u32 y) {
    if (mean_above(a, x, y)) return true;
    if (mean_above(a, y, x)) return false;
    if (a.length[x] != a.length[y]) return a.length[x] > a.length[y];
    return x < y;
}

// distinct targets of the run with source x, counted by the wave up to more than `cap`
__device__ inline u32 wave_degree(const SbArgs& a, u32 x, u32 lane, u32 cap) {
    const u64 i0 = lower_bound(a, (u64)x << 32);
    u32 n = 0;
    for (u64 b = i0; b < a.n_arcs && n <= cap; b += 64) {
        const u64 i = b + lane;
        const u64 k = i < a.n_arcs ? a.sk[i] : ~0ull;
        const bool mine = i < a.n_arcs && (u32)(k >> 32) == x;
        const bool first = mine && (i == i0 || a.sk[i - 1] != k);
        n += (u32)__popcll(__ballot(first));
        if (__ballot(mine) != ~0ull) break;
    }
    return n;
}

// One field of the visited set: slot i lives in lane i & 63, in register a (i < 64) or b.  Two named registers and selects, never an array indexed at run time: the
// compiler would move such an array out of the registers into per-thread LDS.
struct Pair { u32 a, b; };
__device__ __forceinline__ u32 pick(const Pair& f, u32 j) { return j ? f.b : f.a; }
__device__ __forceinline__ void put(Pair& f, u32 j, u32 v) { f.a = j ? f.a : v; f.b = j ? v : f.b; }
struct Slots {
    Pair ov, pend, vb, best, bu;   // oriented unitig; in-arcs not yet seen; val (of the best in-neighbour until pend == 0, then the vertex's own); best: slot and unitig
    u32 expanded, kept;            // bit j: register j
    u32 n;                         // slots in use (uniform)
};
__device__ __forceinline__ u32 slot_get(const Pair& f, u32 slot) { return (u32)__shfl((int)pick(f, slot >> 6), (int)(slot & 63)); }
__device__ __forceinline__ bool in_use(const Slots& q, u32 lane, u32 j) { return lane + 64 * j < q.n; }

// Kahn's traversal from the oriented unitig ov_s.  SB_YES: (s, *t_slot) bounds a superbubble that fits, its interior = the expanded slots; SB_NO: it bounds none,
// or one that does not fit; SB_DEFECT.  Every branch on the way is taken by the whole wave.
__device__ __forceinline__ u32 traverse(const SbArgs& a, u32 ov_s, u32 lane, Slots& q, u32* t_slot) {
    const u32 u_s = ov_s >> 1;
    q.n = 0; q.expanded = 0; q.kept = 0;
    q.ov = q.pend = q.vb = q.best = q.bu = Pair{NONE, NONE};
    u64 sum_nodes = 0, sum_bases = 0;
    u32 cur = SLOT_S;
    for (u32 round = 0; round <= MAXU; ++round) {                 // s and at most MAXU interior vertices: with the slots, (f)
        u32 ov_y = ov_s, vb_y = NONE;
        if (cur != SLOT_S) {
            ov_y = slot_get(q.ov, cur); vb_y = slot_get(q.vb, cur);
            const u32 u = ov_y >> 1;
            sum_nodes += entries(a, u); sum_bases += a.length[u];
            if ((a.max_nodes && sum_nodes > a.max_nodes) || (a.max_bases && sum_bases > a.max_bases)) return SB_NO;
            if (lane == (cur & 63)) q.expanded |= 1u << (cur >> 6);
        }
        const u32 u_y = ov_y >> 1, x = exit_of(a, ov_y);
        const u64 i0 = lower_bound(a, (u64)x << 32);
        u32 n_out = 0;
        for (u64 b = i0; b < a.n_arcs; b += 64) {
            const u64 i = b + lane;
            const u64 k = i < a.n_arcs ? a.sk[i] : ~0ull;
            const bool mine = i < a.n_arcs && (u32)(k >> 32) == x;
            const bool first = mine && (i == i0 || a.sk[i - 1] != k);      // parallel records and duplicates are one arc
            for (u64 m = __ballot(first); m; m &= m - 1) {
                const u32 w = (u32)__shfl((int)(u32)k, __ffsll((long long)m) - 1);
                ++n_out;
                u32 ov_w;
                if (!oriented_at(a, w, &ov_w)) return SB_DEFECT;
                const u32 u_w = ov_w >> 1;
                if (u_w == u_s) return SB_NO;                     // back to s (c), or its complement (d)
                const u64 h0 = __ballot(in_use(q, lane, 0) && (q.ov.a >> 1) == u_w), h1 = __ballot(in_use(q, lane, 1) && (q.ov.b >> 1) == u_w);
                u32 f;
                if (h0 | h1) {
                    f = h0 ? (u32)__ffsll((long long)h0) - 1 : 64 + (u32)__ffsll((long long)h1) - 1;
                    if (slot_get(q.ov, f) != ov_w) return SB_NO;  // the complement is inside (d)
                } else {
                    if (q.n == CAP) return SB_NO;                 // (f)
                    f = q.n++;
                    const u32 deg = wave_degree(a, w ^ 1u, lane, CAP);      // in-neighbours lie in I and s: more than 65 never become ready
                    if (lane == (f & 63)) { put(q.ov, f >> 6, ov_w); put(q.pend, f >> 6, deg); put(q.best, f >> 6, NONE); }
                }
                if (lane == (f & 63)) {                           // the owner of slot f: the fields out of their registers, updated, and back
                    const u32 j = f >> 6;
                    u32 best = pick(q.best, j), vb = pick(q.vb, j), bu = pick(q.bu, j), pend = pick(q.pend, j);
                    if (best == NONE || val_above(a, vb_y, vb) || (!val_above(a, vb, vb_y) && beats(a, u_y, bu))) { best = cur; vb = vb_y; bu = u_y; }
                    if (pend != 0 && --pend == 0 && (vb == NONE || mean_above(a, vb, u_w))) vb = u_w;      // val = min(mean, val(best))
                    put(q.best, j, best); put(q.vb, j, vb); put(q.bu, j, bu); put(q.pend, j, pend);
                }
            }
            if (__ballot(mine) != ~0ull) break;
        }
        if (n_out == 0) return SB_NO;                             // a dead end (a)
        u64 r[2]; bool waiting = false;
        for (u32 j = 0; j < 2; ++j) {
            const bool used = in_use(q, lane, j), done = (q.expanded >> j) & 1u;
            r[j] = __ballot(used && !done && pick(q.pend, j) == 0);
            waiting |= __ballot(used && pick(q.pend, j) != 0) != 0;
        }
        const u32 n_ready = (u32)(__popcll(r[0]) + __popcll(r[1]));
        if (n_ready == 0) return SB_NO;                           // an in-arc from outside, or a cycle
        const u32 next = r[0] ? (u32)__ffsll((long long)r[0]) - 1 : 64 + (u32)__ffsll((long long)r[1]) - 1;
        if (n_ready == 1 && !waiting) {
            const u32 ov_t = slot_get(q.ov, next);
            const u64 back = ((u64)exit_of(a, ov_t) << 32) | entry_of(a, ov_s), at = lower_bound(a, back);
            if (at < a.n_arcs && a.sk[at] == back) return SB_NO;  // t -> s closes a cycle (c)
            *t_slot = next;
            return SB_YES;
        }
        cur = next;
    }
    return SB_NO;
}

__global__ __launch_bounds__(256) void sb_cand_kernel(SbArgs a) {
    const u64 ov = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (ov >= 2 * a.U || a.circ[ov >> 1]) return;
    const u32 x = exit_of(a, (u32)ov);
    u32 n = 0; u64 last = 0;
    for (u64 i = lower_bound(a, (u64)x << 32); i < a.n_arcs && (u32)(a.sk[i] >> 32) == x && n < 2; ++i) {
        const u64 k = a.sk[i];
        if (n && k == last) continue;
        last = k; ++n;
    }
    if (n < 2) return;
    const u32 at = atomicAdd(a.sctr, 1u);
    if (at < 2 * a.U) a.cand[at] = (u32)ov;
}

__global__ __launch_bounds__(256) void sb_find_kernel(SbArgs a) {
    const u32 lane = threadIdx.x & 63, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    const u64 n_cand = a.sctr[0] < 2 * a.U ? a.sctr[0] : 2 * a.U;
    Slots q;
    for (u64 c = wave; c < n_cand; c += n_waves) {
        const u32 ov_s = a.cand[c];
        if (ov_s >= 2 * a.U) { if (lane == 0) atomicOr(a.sctr + 2, 1u); continue; }
        u32 t_slot = 0;
        const u32 got = traverse(a, ov_s, lane, q, &t_slot);
        if (got == SB_DEFECT && lane == 0) atomicOr(a.sctr + 2, 1u);
        if (got != SB_YES) continue;
        for (u32 j = 0; j < 2; ++j)
            if (in_use(q, lane, j) && ((q.expanded >> j) & 1u)) a.J[pick(q.ov, j) >> 1] = 1;      // plain stores of one constant
        const u32 u_t = slot_get(q.ov, t_slot) >> 1;
        if ((ov_s >> 1) < u_t && lane == 0) {                     // the canonical reading: (d) makes the two unitigs different
            const u32 at = atomicAdd(a.sctr + 1, 1u);
            if (at < 2 * a.U) a.app[at] = ov_s;
        }
    }
}

__global__ __launch_bounds__(256) void sb_decide_kernel(SbArgs a) {
    const u32 lane = threadIdx.x & 63, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    const u64 n_app = a.sctr[1] < 2 * a.U ? a.sctr[1] : 2 * a.U;
    Slots q;
    for (u64 c = wave; c < n_app; c += n_waves) {
        const u32 ov_s = a.app[c];
        if (ov_s >= 2 * a.U) { if (lane == 0) atomicOr(a.sctr + 2, 1u); continue; }
        if (a.J[ov_s >> 1]) continue;                             // s lies inside a fitting bubble
        u32 t_slot = 0;
        if (traverse(a, ov_s, lane, q, &t_slot) != SB_YES) { if (lane == 0) atomicOr(a.sctr + 2, 1u); continue; }
        if (a.J[slot_get(q.ov, t_slot) >> 1]) continue;           // t does
        u32 cur = t_slot; bool home = false;
        for (u32 step = 0; step <= CAP && !home; ++step) {        // t, best(t), best(best(t)), ... back to s
            const u32 b = slot_get(q.best, cur);
            if (b == SLOT_S) { home = true; break; }
            if (b >= q.n) break;
            if (lane == (b & 63)) q.kept |= 1u << (b >> 6);
            cur = b;
        }
        if (!home) { if (lane == 0) atomicOr(a.sctr + 2, 1u); continue; }
        for (u32 j = 0; j < 2; ++j)
            if (in_use(q, lane, j) && ((q.expanded >> j) & 1u) && !((q.kept >> j) & 1u)) a.rem[pick(q.ov, j) >> 1] = 1;
    }
}

__global__ __launch_bounds__(256) void sb_count_kernel(SbArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    count_to(a.ctr, u < a.U && a.rem[u]);
}

}  // namespace

hipError_t superbubbles_run(UnitigBuffers* B, const UnitigResult& ul, u32 n2x, const u32* uhead, const u32* utail, u32 max_nodes, u64 max_bases, u8* rem, u32* ctr,
                            hipStream_t s, const u32** defect_flag) {
    const u64 U = ul.n_unitigs;
    GHIP(B->sb_cand.ensure(2 * U * 4)); GHIP(B->sb_app.ensure(2 * U * 4)); GHIP(B->sb_J.ensure(U)); GHIP(B->sb_ctr.ensure(12));
    GHIP(hipMemsetAsync(B->sb_J.p, 0, U, s));
    GHIP(hipMemsetAsync(B->sb_ctr.p, 0, 12, s));
    GHIP(hipMemsetAsync(rem, 0, U, s));
    SbArgs a; memset(&a, 0, sizeof a);
    a.n2x = n2x; a.U = U; a.n_arcs = B->n_arcs; a.sk = B->skeys.as<u64>(); a.P = B->Pfin; a.flag = B->flag.as<u32>(); a.uid = B->uid.as<u32>(); a.uhead = uhead; a.utail = utail;
    a.offsets = ul.offsets; a.length = ul.length; a.kc = ul.kc_sum; a.circ = ul.circular; a.max_nodes = max_nodes; a.max_bases = max_bases;
    a.cand = B->sb_cand.as<u32>(); a.app = B->sb_app.as<u32>(); a.J = B->sb_J.as<u8>(); a.sctr = B->sb_ctr.as<u32>(); a.rem = rem; a.ctr = ctr;
    const u64 want = (2 * U + 3) / 4;                            // four waves per workgroup; a fixed grid strides over the lists, whose lengths stay on the device
    const unsigned gw = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(sb_cand_kernel, dim3(grid_for(2 * U)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sb_find_kernel, dim3(gw), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sb_decide_kernel, dim3(gw), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sb_count_kernel, dim3(grid_for(U)), dim3(256), 0, s, a);
    *defect_flag = a.sctr + 2;
    return hipGetLastError();
}
