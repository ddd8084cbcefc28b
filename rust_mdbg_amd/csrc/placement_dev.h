// placement_dev.h — what the kernels over a placement share on the device (placement.hip, read_paths.hip, junctions.hip, transits.hip): the packed vertices,
// pairs and keys of include/mdbg_hip.h (mdbg_graph_junctions), the tests on two neighbouring place codes, the defect mask and the per-workgroup counts.
// Header-only, inline device functions and no kernel.
//
// A vertex (u, j, s) is the number v = 2 * (offsets[u] + j) + s < 2^31; a pair x -> y is the u64 vx << 32 | vy, its mirror (vy ^ 1) << 32 | (vx ^ 1), its KEY the
// smaller of the two: the order of the packed keys is the definition's order of keys.
#pragma once
#include "graph_common.h"
#include "placement.h"

namespace {

constexpr u64 JX_NO_KEY = ~0ull;       // (a key is below 2^63)

__device__ inline u64 pair_of(u32 vx, u32 vy) { return (u64)vx << 32 | vy; }
__device__ inline u64 mirror_of_pair(u64 p) { return (u64)((u32)p ^ 1u) << 32 | ((u32)(p >> 32) ^ 1u); }
__device__ inline u64 key_of_pair(u32 vx, u32 vy) {
    const u64 a = (u64)vx << 32 | vy, b = (u64)(vy ^ 1u) << 32 | (vx ^ 1u);
    return a < b ? a : b;
}
__device__ inline u32 vertex_of_code(u32 c) { return (c & ~RP_STRAND) << 1 | c >> 31; }
// the first position in sorted[0, n) whose key is >= key
__device__ inline u64 lower_bound(const u64* sorted, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (sorted[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// c = code[t] of the range that starts at index i0: is the window placed, and the one in front of it too, in the same read?  *pc <- code[t - 1] then.
// (The range starts at a read's first index.)
__device__ inline bool adjacent_in_read(const u32* code, const u64* roff, const u32* mread, u64 i0, u64 t, u32 c, u32* pc) {
    if (c == RP_NONE || t == 0) return false;
    const u64 i = i0 + t;
    if (i <= roff[mread[i]]) return false;
    *pc = code[t - 1];
    return *pc != RP_NONE;
}
// code[t - 1] -> code[t], both placed: a link of the definition?
__device__ inline bool is_link_of_codes(u32 pc, u32 c, const u32* unitig_of_entry) {
    const u32 e = c & ~RP_STRAND, pe = pc & ~RP_STRAND;
    return !((pc ^ c) & RP_STRAND) && unitig_of_entry[e] == unitig_of_entry[pe] && (c & RP_STRAND ? pe == e + 1 : e == pe + 1);
}
// What the pair code[t - 1] -> code[t] is, for every stage that asks (junctions.hip, transits.hip, alignments.hip): PAIR_NONE no adjacent pair (adjacent_in_read),
// PAIR_LINK a link, PAIR_EXPLAINED a crossing whose key is some record's key, PAIR_MISSING a crossing on no record.  A crossing leaves its key in *key and, explained,
// in *at the first position of the key's run in rkey_sorted[0, R): the key's counter slot, and rec_sorted[*at] its smallest record.
enum PairKind : u32 { PAIR_NONE = 0, PAIR_LINK, PAIR_EXPLAINED, PAIR_MISSING };
__device__ inline PairKind classify_pair(const u32* code, const u64* roff, const u32* mread, u64 i0, u64 t, u32 c, const u32* unitig_of_entry, const u64* rkey_sorted, u64 R,
                                         u64* key, u64* at) {
    u32 pc;
    if (!adjacent_in_read(code, roff, mread, i0, t, c, &pc)) return PAIR_NONE;
    if (is_link_of_codes(pc, c, unitig_of_entry)) return PAIR_LINK;
    *key = key_of_pair(vertex_of_code(pc), vertex_of_code(c));
    *at = lower_bound(rkey_sorted, R, *key);
    return *at < R && rkey_sorted[*at] == *key ? PAIR_EXPLAINED : PAIR_MISSING;
}
__device__ inline void set_defect(u64* counters, u32 what) { atomicOr((unsigned long long*)(counters + RP_C_DEFECT), (unsigned long long)what); }
// the workgroup's counts (256 threads, NC of them per thread): one atomic each on counters[first .. first + NC).  cnt[] is reduced IN PLACE: on return the first
// lane of every wave holds its wave's sums (the other lanes partial ones).  resolve_kernel (placement.hip) relies on that for a second counter; keep it
template <int NC> __device__ inline void block_add(u32 (&cnt)[NC], u64* counters, int first) {
    __shared__ u32 wsum[NC][4];
#pragma unroll
    for (int q = 0; q < NC; ++q) for (int d = 32; d; d >>= 1) cnt[q] += __shfl_down(cnt[q], d, 64);
    if ((threadIdx.x & 63) == 0) for (int q = 0; q < NC; ++q) wsum[q][threadIdx.x >> 6] = cnt[q];
    __syncthreads();
    if (threadIdx.x < NC) {
        const u32 v = wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
        if (v) atomicAdd((unsigned long long*)(counters + first + threadIdx.x), (unsigned long long)v);
    }
}

}  // namespace
