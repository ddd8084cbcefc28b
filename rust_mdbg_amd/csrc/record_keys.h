// record_keys.h — the packed vertices, pairs and keys of include/mdbg_hip.h (mdbg_graph_junctions) and the kernel that writes the key of every edge record: what the
// junction stage (junctions.hip) and the transit stage (transits.hip) share on the device.  Header-only; each translation unit gets its own copy of the kernel.
//
// A vertex (u, j, s) is the number v = 2 * (offsets[u] + j) + s < 2^31; a pair x -> y is the u64 vx << 32 | vy, its mirror (vy ^ 1) << 32 | (vx ^ 1), its KEY the
// smaller of the two: the order of the packed keys is the definition's order of keys.
#pragma once
#include "graph_common.h"
#include "read_paths.h"

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
// code[t - 1] -> code[t], both placed: a link of the definition?
__device__ inline bool is_link_of_codes(u32 pc, u32 c, const u32* unitig_of_entry) {
    const u32 e = c & ~RP_STRAND, pe = pc & ~RP_STRAND;
    return !((pc ^ c) & RP_STRAND) && unitig_of_entry[e] == unitig_of_entry[pe] && (c & RP_STRAND ? pe == e + 1 : e == pe + 1);
}

struct RecordKeyArgs {
    u64 U, R; const u64* offsets;
    const u32* n1; const u8* o1; const u32* n2; const u8* o2;
    u64* rkey; u32* rec;               // [R] each
    u64* defect; u64 defect_bit;       // a record that names a unitig outside the list: *defect |= defect_bit, its key is JX_NO_KEY
};

// one thread per edge record r: rkey[r] = the record's key, rec[r] = r
__global__ __launch_bounds__(256) void record_key_kernel(RecordKeyArgs a) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    const u32 n1 = a.n1[r], n2 = a.n2[r];
    a.rec[r] = (u32)r;
    if (n1 >= a.U || n2 >= a.U) {
        atomicOr((unsigned long long*)a.defect, (unsigned long long)a.defect_bit);
        a.rkey[r] = JX_NO_KEY;
        return;
    }
    const bool m1 = a.o1[r] == '-', m2 = a.o2[r] == '-';
    const u64 e1 = m1 ? a.offsets[n1] : a.offsets[n1 + 1] - 1;      // the record leaves n1 at its last entry ('+') or, walked backwards, at its first
    const u64 e2 = m2 ? a.offsets[n2 + 1] - 1 : a.offsets[n2];      // and enters n2 at its first entry ('+') or its last
    a.rkey[r] = key_of_pair((u32)(e1 << 1) | (u32)m1, (u32)(e2 << 1) | (u32)m2);
}

}  // namespace
