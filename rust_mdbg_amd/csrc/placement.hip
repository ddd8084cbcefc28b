// placement.hip — the placement every read-evidence stage starts with, on the GPU (gfx950).  Interface and what it is for: placement.h.
//
//   (memset)            the caller's counters <- 0, entry_of_row <- NONE
//   entry_kernel        one thread per list entry e: the row of node[e] by binary search (rows are in index order) gets e; unitig_of_entry[e] by binary
//                       search in offsets.  A node index that is no row sets RP_DEFECT_ENTRY
//   record_key_kernel   (with records) one thread per edge record r: rkey[r] = the record's key, rec[r] = r.  A record that names a unitig outside the list sets
//                       JX_DEFECT_EDGE, its key is JX_NO_KEY
//   (rocPRIM)           (with records) sort_pairs(rkey, rec): equal keys are one run; stable, so a key's run starts at its smallest record
//   place_windows_kernel  (place_windows.hip, through the WindowPlacer) code[t] = entry | strand << 31 of the window that starts at index i0 + t, or NONE
//
// No loop but the two binary searches; the number of launches is fixed.  Per context, once: 4 bytes per row of the table and per entry of the list (the maps),
// 4 per minimizer index of the range (code), 24 per edge record (the keys and record numbers, both sorted and not), the counter block and the sort's temporary.
#include <cstring>

#include "placement_dev.h"

struct PlacementBuffers {
    Buf entry_of_row, unitig_of_entry, code, counters, tmp;
    Buf rkey, rkey_sorted, rec, rec_sorted;                // per edge record
};

namespace {

struct EntryArgs {
    u64 U, N, n_rows; const u64* offsets; const u32* node; const u32* index;
    u32* entry_of_row; u32* unitig_of_entry; u64* counters;
};
__global__ __launch_bounds__(256) void entry_kernel(EntryArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.N) return;
    {   // the unitig that holds entry e: the last u with offsets[u] <= e
        u64 lo = 0, hi = a.U - 1;
        while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (a.offsets[mid] <= e) lo = mid; else hi = mid - 1; }
        a.unitig_of_entry[e] = (u32)lo;
    }
    const u32 idx = a.node[e];
    u64 lo = 0, hi = a.n_rows;                 // as row_of (unitigs.hip)
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.index[mid] < idx) lo = mid + 1; else hi = mid; }
    if (lo < a.n_rows && a.index[lo] == idx) a.entry_of_row[lo] = (u32)e;
    else set_defect(a.counters, RP_DEFECT_ENTRY);
}

struct RecordKeyArgs {
    u64 U, R; const u64* offsets;
    const u32* n1; const u8* o1; const u32* n2; const u8* o2;
    u64* rkey; u32* rec;               // [R] each
    u64* counters;
};
__global__ __launch_bounds__(256) void record_key_kernel(RecordKeyArgs a) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    const u32 n1 = a.n1[r], n2 = a.n2[r];
    a.rec[r] = (u32)r;
    if (n1 >= a.U || n2 >= a.U) {
        set_defect(a.counters, JX_DEFECT_EDGE);
        a.rkey[r] = JX_NO_KEY;
        return;
    }
    const bool m1 = a.o1[r] == '-', m2 = a.o2[r] == '-';
    const u64 e1 = m1 ? a.offsets[n1] : a.offsets[n1 + 1] - 1;      // the record leaves n1 at its last entry ('+') or, walked backwards, at its first
    const u64 e2 = m2 ? a.offsets[n2 + 1] - 1 : a.offsets[n2];      // and enters n2 at its first entry ('+') or its last
    a.rkey[r] = key_of_pair((u32)(e1 << 1) | (u32)m1, (u32)(e2 << 1) | (u32)m2);
}

}  // namespace

PlacementBuffers* placement_buffers_create() { return new PlacementBuffers(); }
void placement_buffers_destroy(PlacementBuffers* b) { delete b; }

hipError_t placement_reserve(PlacementBuffers* P, const UnitigResult& ul, u64 n_rows, const ReadPathRange& rg, bool with_records) {
    const u64 U = ul.n_unitigs, N = ul.n_entries, R = with_records ? ul.edges.n : 0, n_idx = rg.i1 - rg.i0;
    if (U == 0 || N == 0 || n_rows == 0 || N >= (1ull << 30) || n_rows >= (1ull << 30) || n_idx >= 0xFFFFFFF0ull || R >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    GHIP(P->counters.ensure(PLACEMENT_COUNTERS * 8));
    GHIP(P->entry_of_row.ensure(n_rows * 4)); GHIP(P->unitig_of_entry.ensure(N * 4)); GHIP(P->code.ensure(n_idx * 4 + 4));
    if (!with_records) return hipSuccess;
    GHIP(P->rkey.ensure(R * 8 + 8)); GHIP(P->rkey_sorted.ensure(R * 8 + 8)); GHIP(P->rec.ensure(R * 4 + 4)); GHIP(P->rec_sorted.ensure(R * 4 + 4));
    if (R) {
        size_t tb = 0;
        GHIP(rocprim::radix_sort_pairs(nullptr, tb, P->rkey.as<const u64>(), P->rkey_sorted.as<u64>(), P->rec.as<const u32>(), P->rec_sorted.as<u32>(), (size_t)R, 0u, 64u, hipStream_t(nullptr)));
        GHIP(P->tmp.ensure(tb + 256));
    }
    return hipSuccess;
}

hipError_t placement_queue(PlacementBuffers* P, const UnitigResult& ul, const u32* index, u64 n_rows, const ReadPathRange& rg, bool with_records, u32 n_counters,
                           const WindowPlacer& placer, hipStream_t s, PlacementView* view) {
    memset(view, 0, sizeof *view);
    const u64 R = with_records ? ul.edges.n : 0;
    if (n_counters < RP_C_N || n_counters > PLACEMENT_COUNTERS) return hipErrorInvalidValue;
    u64* counters = P->counters.as<u64>();
    GHIP(hipMemsetAsync(counters, 0, (size_t)n_counters * 8, s));
    GHIP(hipMemsetAsync(P->entry_of_row.p, 0xFF, n_rows * 4, s));
    const EntryArgs ea{ul.n_unitigs, ul.n_entries, n_rows, ul.offsets, ul.node, index, P->entry_of_row.as<u32>(), P->unitig_of_entry.as<u32>(), counters};
    hipLaunchKernelGGL(entry_kernel, dim3(grid_for(ea.N)), dim3(256), 0, s, ea);
    if (R) {
        const RecordKeyArgs rk{ul.n_unitigs, R, ul.offsets, ul.edges.n1, ul.edges.o1, ul.edges.n2, ul.edges.o2, P->rkey.as<u64>(), P->rec.as<u32>(), counters};
        hipLaunchKernelGGL(record_key_kernel, dim3(grid_for(R)), dim3(256), 0, s, rk);
        GHIP(hipGetLastError());
        GHIP(sort_pairs(P->tmp, (const u64*)rk.rkey, P->rkey_sorted.as<u64>(), (const u32*)rk.rec, P->rec_sorted.as<u32>(), (size_t)R, 0u, 64u, s));
    }
    const ReadPathPlan plan{ea.entry_of_row, n_rows, ul.ori, P->code.as<u32>(), counters};
    placer.place(placer.ctx, plan, s);
    *view = PlacementView{ea.entry_of_row, ea.unitig_of_entry, plan.code, counters, P->rkey_sorted.as<u64>(), P->rec_sorted.as<u32>(), R};
    return hipGetLastError();
}
