// junctions.hip — read support per junction of the current unitig list, on the GPU (gfx950): how many resident reads cross each edge record, and which
// crossings lie on no record.  Definition: include/mdbg_hip.h (mdbg_graph_junctions).  Input: the device arrays of a unitig list (unitigs.hip) with its edge
// records, the store's read offsets and minimizer -> read map, and the placement with records (placement.h): unitig_of_entry, the per-index place codes
// (code[t] = global entry | strand << 31 or NONE) and the edge records in key order, in the context's one placement scratch.
//
// Vertices, pairs and keys are packed as placement_dev.h says: the order of the packed keys is the definition's order of keys.
//
//   (memset)            the counter slots <- 0
//   (placement_queue)   the counters and the map zeroed, entry_kernel, record_key_kernel, sort_pairs(rkey, rec): equal keys are one run, the run's first
//                       position is the key's counter slot; place_windows_kernel: code[]
//   cross_kernel       one thread per minimizer index t of the range: code[t - 1] -> code[t], both placed and in one read, is a link or a crossing; a crossing's
//                       key is searched in the sorted record keys: found, one integer atomic on the key's slot; not found, the key goes to mkey[t] (else ~0).
//                       The four counts are reduced per workgroup: one atomic each
//   (rocPRIM)           sort_keys(mkey): the missing crossings in key order, the ~0 of every other index behind them
//   head_kernel         flag[t] = 1 iff sorted mkey[t] is a key and differs from the one in front;  (rocPRIM) pos = exclusive scan of flag
//   missing_kernel      a head unpacks its key into the six columns at pos[t]; its count is the length of its run (the first greater key, by binary search)
//   support_kernel      one thread per sorted record: support[rec] = the slot at the first position of its key
//
// All sums are integers and every position comes from a sort or a scan: two calls give identical arrays.  No loop but the binary searches; the number of
// launches is fixed.  Per minimizer index of the range, beside the placement's 4: 21 bytes of temporaries (mkey and its sorted copy 16, flag 1, pos 4) and 26
// bytes of missing columns, sized for the worst case (every pair a missing crossing of its own) because their number is known only on the device.  Per edge
// record, beside the placement's 24: the counter slot 8 and the support 8.
#include <cstring>

#include "junctions.h"
#include "placement_dev.h"

struct JunctionBuffers {
    Buf slot;                                              // per edge record
    Buf mkey, mkey_sorted, flag, pos, tmp;                 // per minimizer index
    Buf support, mu1, me1, ms1, mu2, me2, ms2, mcount;     // the result
    StageTimer timer;
};

namespace {

struct JxArgs {
    u64 R; const u64* offsets; const u32* unitig_of_entry;
    const u64* rkey_sorted; const u32* rec_sorted; u64* slot;
    const u64* roff; const u32* mread; u64 i0, n_idx;
    const u32* code; u64* mkey; const u64* mkey_sorted; u8* flag; const u32* pos; u64* counters;
    u64* support; u32* mu1; u32* me1; u8* ms1; u32* mu2; u32* me2; u8* ms2; u64* mcount;
};

__global__ __launch_bounds__(256) void cross_kernel(JxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[4] = {0, 0, 0, 0};         // adjacent, links, explained, missing crossings
    if (t < a.n_idx) {
        u64 missing = JX_NO_KEY;
        const u32 c = a.code[t];
        u64 key = 0, p = 0;
        const PairKind kind = classify_pair(a.code, a.roff, a.mread, a.i0, t, c, a.unitig_of_entry, a.rkey_sorted, a.R, &key, &p);
        if (kind != PAIR_NONE) cnt[0] = 1;
        if (kind == PAIR_LINK) cnt[1] = 1;
        else if (kind == PAIR_EXPLAINED) { atomicAdd((unsigned long long*)(a.slot + p), 1ull); cnt[2] = 1; }
        else if (kind == PAIR_MISSING) { missing = key; cnt[3] = 1; }
        a.mkey[t] = missing;
    }
    block_add<4>(cnt, a.counters, JX_C_ADJACENT);
}

__global__ __launch_bounds__(256) void head_kernel(JxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u64 key = a.mkey_sorted[t];
    a.flag[t] = key != JX_NO_KEY && (t == 0 || a.mkey_sorted[t - 1] != key);
}

__global__ __launch_bounds__(256) void missing_kernel(JxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u32 f = a.flag[t], d = a.pos[t];
    if (t == a.n_idx - 1) a.counters[JX_C_MISSING] = (u64)d + f;
    if (!f) return;
    const u64 key = a.mkey_sorted[t];
    const u32 vx = (u32)(key >> 32), vy = (u32)key;
    const u32 ex = vx >> 1, ey = vy >> 1;                  // (both came out of code[]: entries of the list)
    const u32 ux = a.unitig_of_entry[ex], uy = a.unitig_of_entry[ey];
    a.mu1[d] = ux; a.me1[d] = (u32)(ex - a.offsets[ux]); a.ms1[d] = (u8)(vx & 1u);
    a.mu2[d] = uy; a.me2[d] = (u32)(ey - a.offsets[uy]); a.ms2[d] = (u8)(vy & 1u);
    a.mcount[d] = lower_bound(a.mkey_sorted, a.n_idx, key + 1) - t;
}

__global__ __launch_bounds__(256) void support_kernel(JxArgs a) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.R) return;
    const u32 r = a.rec_sorted[p];
    if (r < a.R) a.support[r] = a.slot[lower_bound(a.rkey_sorted, a.R, a.rkey_sorted[p])];
}

JxArgs args_of(JunctionBuffers* B, const PlacementView& V, const UnitigResult& ul, const ReadPathRange& rg) {
    JxArgs a; memset(&a, 0, sizeof a);
    a.R = V.R; a.offsets = ul.offsets; a.unitig_of_entry = V.unitig_of_entry;
    a.rkey_sorted = V.rkey_sorted; a.rec_sorted = V.rec_sorted; a.slot = B->slot.as<u64>();
    a.roff = rg.roff; a.mread = rg.mread; a.i0 = rg.i0; a.n_idx = rg.i1 - rg.i0;
    a.code = V.code; a.mkey = B->mkey.as<u64>(); a.mkey_sorted = B->mkey_sorted.as<u64>(); a.flag = B->flag.as<u8>(); a.pos = B->pos.as<u32>(); a.counters = V.counters;
    a.support = B->support.as<u64>(); a.mu1 = B->mu1.as<u32>(); a.me1 = B->me1.as<u32>(); a.ms1 = B->ms1.as<u8>(); a.mu2 = B->mu2.as<u32>(); a.me2 = B->me2.as<u32>(); a.ms2 = B->ms2.as<u8>();
    a.mcount = B->mcount.as<u64>();
    return a;
}

}  // namespace

JunctionBuffers* junction_buffers_create() { return new JunctionBuffers(); }
void junction_buffers_destroy(JunctionBuffers* b) { delete b; }

hipError_t junctions_run(JunctionBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const u32* index, u64 n_rows, const ReadPathRange& rg, const WindowPlacer& placer,
                         hipStream_t s, JunctionResult* out, const OriginMap& om) {
    memset(out, 0, sizeof *out);
    const u64 R = ul.edges.n, n_idx = rg.i1 - rg.i0;
    // every buffer first: growing one may wait for the device (graph_common.h), and nothing of this call is queued yet
    GHIP(placement_reserve(P, ul, n_rows, rg, true, om));
    GHIP(B->slot.ensure(R * 8 + 8)); GHIP(B->support.ensure(R * 8 + 8));
    GHIP(B->mkey.ensure(n_idx * 8 + 8)); GHIP(B->mkey_sorted.ensure(n_idx * 8 + 8)); GHIP(B->flag.ensure(n_idx + 4)); GHIP(B->pos.ensure(n_idx * 4 + 4));
    GHIP(B->mu1.ensure(n_idx * 4 + 4)); GHIP(B->me1.ensure(n_idx * 4 + 4)); GHIP(B->ms1.ensure(n_idx + 4)); GHIP(B->mu2.ensure(n_idx * 4 + 4)); GHIP(B->me2.ensure(n_idx * 4 + 4)); GHIP(B->ms2.ensure(n_idx + 4));
    GHIP(B->mcount.ensure(n_idx * 8 + 8));
    if (n_idx) {   // the larger temporary of the stage's two rocPRIM calls, so that `tmp` does not grow between them
        size_t tb = 0, most = 0;
        GHIP(rocprim::radix_sort_keys(nullptr, most, B->mkey.as<u64>(), B->mkey_sorted.as<u64>(), (size_t)n_idx, 0u, 64u, s));
        GHIP(rocprim::exclusive_scan(nullptr, tb, B->flag.as<u8>(), B->pos.as<u32>(), 0u, (size_t)n_idx, rocprim::plus<u32>(), s)); if (tb > most) most = tb;
        GHIP(B->tmp.ensure(most + 256));
    }
    GHIP(B->timer.start(s));
    if (R) GHIP(hipMemsetAsync(B->slot.p, 0, R * 8, s));
    PlacementView V;
    GHIP(placement_queue(P, ul, index, n_rows, rg, true, JX_C_N, placer, s, &V, om));
    const JxArgs a = args_of(B, V, ul, rg);
    if (a.n_idx) {
        const unsigned gi = grid_for(a.n_idx);
        hipLaunchKernelGGL(cross_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(hipGetLastError());
        GHIP(sort_keys(B->tmp, (const u64*)a.mkey, B->mkey_sorted.as<u64>(), (size_t)a.n_idx, 0u, 64u, s));
        hipLaunchKernelGGL(head_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(excl_scan(B->tmp, (const u8*)a.flag, B->pos.as<u32>(), (size_t)a.n_idx, s));
        hipLaunchKernelGGL(missing_kernel, dim3(gi), dim3(256), 0, s, a);
    }
    if (a.R) hipLaunchKernelGGL(support_kernel, dim3(grid_for(a.R)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    u64 h[JX_C_N];
    GHIP(B->timer.stop_and_read(h, a.counters, sizeof h, s, &out->ms));
    out->defect = (u32)h[RP_C_DEFECT];
    if (out->defect) return hipSuccess;
    out->n_reads = rg.n_reads; out->n_adjacent = h[JX_C_ADJACENT]; out->n_links = h[JX_C_LINKS]; out->n_crossings = h[JX_C_ADJACENT] - h[JX_C_LINKS];
    out->n_explained = h[JX_C_EXPLAINED]; out->n_missing_crossings = h[JX_C_MISSING_CROSSINGS]; out->n_records = a.R; out->n_missing = h[JX_C_MISSING];
    out->support = a.support; out->missing_unitig1 = a.mu1; out->missing_entry1 = a.me1; out->missing_strand1 = a.ms1;
    out->missing_unitig2 = a.mu2; out->missing_entry2 = a.me2; out->missing_strand2 = a.ms2; out->missing_count = a.mcount;
    return hipSuccess;
}
