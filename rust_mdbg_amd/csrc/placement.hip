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
//
// On a list that holds copies (an OriginMap with copies > 0; definition: include/mdbg_hip.h, "placement on a list that holds copies") the same launches, with
//   (memset)            mult <- 0, the last four counters <- 0
//   entry_kernel<true>  a node index >= X goes through origin[] first; row_of_entry[e] = the row, mult[row] += 1 (the one atomic), entry_of_row[row] = e, read
//                       only where mult == 1, so which writer wins does not matter
//   place_windows_kernel<true>   a row with mult >= 2 gives the ambiguous code row | RP_AMBIGUOUS | rev << 31
// and behind them
//   mark_kernel         one thread per minimizer index t: fwd[t] = t + 1 unless code[t] is ambiguous, else 0; bwd[n - 1 - t] likewise with n - t
//   (rocPRIM)           two inclusive max-scans: fwd[t] - 1 is the nearest non-ambiguous index at or in front of t, n - bwd[n - 1 - t] the nearest at or behind it
//   resolve_kernel      one thread per minimizer index: an ambiguous window takes its two anchors (same read, placed), steps from each along the anchor's unitig
//                       to its own distance, checks the candidate (inside the anchor's unitig, the window's row, the anchor's strand) and rewrites code[t] to
//                       entry | strand << 31 or NONE.  It reads only codes that are not ambiguous, which nobody rewrites: every window decides alone
// Per row 4 more bytes (mult), per entry 4 (row_of_entry), per minimizer index 16 (fwd, bwd and their scans); the scans' temporary is the sort's.
#include <cstring>

#include "placement_dev.h"

struct PlacementBuffers {
    Buf entry_of_row, unitig_of_entry, code, counters, tmp;
    Buf rkey, rkey_sorted, rec, rec_sorted;                // per edge record
    Buf mult, row_of_entry, anchor, anchor_scan;           // with copies: per row, per entry, per minimizer index (fwd and bwd behind each other, twice)
    size_t scan_tmp = 0; u64 scan_n = 0;                   // with copies: what a max-scan over scan_n indices asks of tmp (placement_reserve)
};

namespace {

struct EntryArgs {
    u64 U, N, n_rows; const u64* offsets; const u32* node; const u32* index;
    u32* entry_of_row; u32* unitig_of_entry; u64* counters;
    OriginMap om; u32* row_of_entry; u32* mult;            // COPIES only
};
template <bool COPIES> __global__ __launch_bounds__(256) void entry_kernel(EntryArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.N) return;
    {   // the unitig that holds entry e: the last u with offsets[u] <= e
        u64 lo = 0, hi = a.U - 1;
        while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (a.offsets[mid] <= e) lo = mid; else hi = mid - 1; }
        a.unitig_of_entry[e] = (u32)lo;
    }
    u32 idx = a.node[e];
    if (COPIES) {
        a.row_of_entry[e] = RP_NONE;
        if (idx >= a.om.X) {                   // a copy: the table row it descends from
            if ((u64)(idx - a.om.X) >= a.om.copies) { set_defect(a.counters, RP_DEFECT_ENTRY); return; }
            idx = a.om.origin[idx - a.om.X];
        }
    }
    u64 lo = 0, hi = a.n_rows;                 // as row_of (unitigs.hip)
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.index[mid] < idx) lo = mid + 1; else hi = mid; }
    if (lo < a.n_rows && a.index[lo] == idx) {
        a.entry_of_row[lo] = (u32)e;
        if (COPIES) { a.row_of_entry[e] = (u32)lo; atomicAdd(a.mult + lo, 1u); }
    } else set_defect(a.counters, RP_DEFECT_ENTRY);
}

// ---- a list that holds copies: the anchors of the ambiguous windows ------------------------------------------
struct ResolveArgs {
    u64 N, n_rows, n_idx, i0; const u64* offsets; const u8* ori; const u32* unitig_of_entry; const u32* row_of_entry;
    const u64* roff; const u32* mread;
    u32* code; u32* fwd; u32* bwd; const u32* fwd_scan; const u32* bwd_scan; u64* counters;
};
__device__ inline bool is_ambiguous(u32 c) { return c != RP_NONE && (c & RP_AMBIGUOUS); }
__global__ __launch_bounds__(256) void mark_kernel(ResolveArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const bool amb = is_ambiguous(a.code[t]);
    a.fwd[t] = amb ? 0u : (u32)t + 1u;
    a.bwd[a.n_idx - 1 - t] = amb ? 0u : (u32)(a.n_idx - t);
}
// The candidate of ambiguous window (row, rev) at distance d behind (behind == true) or in front of the anchor with place code ca: its entry, or RP_NONE if it
// is not valid.  Never indexes ori[] / row_of_entry[] outside the anchor's unitig.
__device__ inline u32 candidate(const ResolveArgs& a, u32 ca, u64 d, bool behind, u32 row, u32 rev) {
    const u32 ea = ca & ~RP_STRAND, sa = ca >> 31;
    if (ea >= a.N) return RP_NONE;
    const u32 u = a.unitig_of_entry[ea];
    const u64 first = a.offsets[u], end = a.offsets[u + 1];
    const bool up = behind == (sa == 0);                   // the read walks the unitig upwards on strand 0
    if (up ? d >= end - ea : d > ea - first) return RP_NONE;      // (no wrap, also on a circular unitig)
    const u32 e = up ? ea + (u32)d : ea - (u32)d;
    if (a.row_of_entry[e] != row || (rev ^ (u32)(a.ori[e] == '-')) != sa) return RP_NONE;
    return e | (sa ? RP_STRAND : 0u);
}
__global__ __launch_bounds__(256) void resolve_kernel(ResolveArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[4] = {0, 0, 0, 0};         // ambiguous, resolved, conflicts, unanchored
    if (t < a.n_idx) {
        const u32 c = a.code[t];
        if (is_ambiguous(c)) {
            const u32 row = c & (RP_AMBIGUOUS - 1u), rev = c >> 31;
            const u64 i = a.i0 + t;
            const u32 slot = a.mread[i];
            const u64 rs = a.roff[slot], re = a.roff[slot + 1];          // the anchors lie in [rs, re): adjacent_in_read's test, over a distance
            u32 left = RP_NONE, right = RP_NONE;
            const u32 f = a.fwd_scan[t], b = a.bwd_scan[a.n_idx - 1 - t];
            if (f) {
                const u64 ta = (u64)f - 1;
                if (a.i0 + ta >= rs) { const u32 ca = a.code[ta]; if (ca != RP_NONE) left = candidate(a, ca, t - ta, true, row, rev); }
            }
            if (b) {
                const u64 tb = a.n_idx - b;
                if (a.i0 + tb < re) { const u32 cb = a.code[tb]; if (cb != RP_NONE) right = candidate(a, cb, tb - t, false, row, rev); }
            }
            cnt[0] = 1;
            u32 out = RP_NONE;
            if (left != RP_NONE && right != RP_NONE && left != right) cnt[2] = 1;
            else if (left != RP_NONE || right != RP_NONE) { out = left != RP_NONE ? left : right; cnt[1] = 1; }
            else cnt[3] = 1;
            a.code[t] = out;
        }
    }
    block_add<4>(cnt, a.counters, NP_C_AMBIGUOUS);
    if ((threadIdx.x & 63) == 0 && cnt[1])                 // (block_add has left every wave's sum in its first lane) a resolved window is a placed one
        atomicAdd((unsigned long long*)(a.counters + RP_C_PLACED), (unsigned long long)cnt[1]);
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
void placement_records(const PlacementBuffers* P, const u64** rkey_sorted, const u32** rec_sorted) { *rkey_sorted = P->rkey_sorted.as<u64>(); *rec_sorted = P->rec_sorted.as<u32>(); }

hipError_t placement_reserve(PlacementBuffers* P, const UnitigResult& ul, u64 n_rows, const ReadPathRange& rg, bool with_records, const OriginMap& om) {
    const u64 U = ul.n_unitigs, N = ul.n_entries, R = with_records ? ul.edges.n : 0, n_idx = rg.i1 - rg.i0;
    if (U == 0 || N == 0 || n_rows == 0 || N >= (1ull << 30) || n_rows >= (1ull << 30) || n_idx >= 0xFFFFFFF0ull || R >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    GHIP(P->counters.ensure(PLACEMENT_COUNTERS * 8));
    GHIP(P->entry_of_row.ensure(n_rows * 4)); GHIP(P->unitig_of_entry.ensure(N * 4)); GHIP(P->code.ensure(n_idx * 4 + 4));
    if (om.copies) {
        GHIP(P->mult.ensure(n_rows * 4)); GHIP(P->row_of_entry.ensure(N * 4)); GHIP(P->anchor.ensure(n_idx * 8 + 8)); GHIP(P->anchor_scan.ensure(n_idx * 8 + 8));
        if (n_idx) {
            size_t tb = 0;
            GHIP(rocprim::inclusive_scan(nullptr, tb, P->anchor.as<const u32>(), P->anchor_scan.as<u32>(), (size_t)n_idx, rocprim::maximum<u32>(), hipStream_t(nullptr)));
            GHIP(P->tmp.ensure(tb + 256));
            P->scan_tmp = tb; P->scan_n = n_idx;
        }
    }
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
                           const WindowPlacer& placer, hipStream_t s, PlacementView* view, const OriginMap& om) {
    memset(view, 0, sizeof *view);
    const u64 R = with_records ? ul.edges.n : 0, n_idx = rg.i1 - rg.i0;
    const bool copies = om.copies != 0;
    if (n_counters < RP_C_N || n_counters > PLACEMENT_COUNTERS) return hipErrorInvalidValue;
    u64* counters = P->counters.as<u64>();
    GHIP(hipMemsetAsync(counters, 0, (size_t)n_counters * 8, s));
    GHIP(hipMemsetAsync(P->entry_of_row.p, 0xFF, n_rows * 4, s));
    EntryArgs ea{ul.n_unitigs, ul.n_entries, n_rows, ul.offsets, ul.node, index, P->entry_of_row.as<u32>(), P->unitig_of_entry.as<u32>(), counters, NO_COPIES, nullptr, nullptr};
    if (copies) {
        GHIP(hipMemsetAsync(counters + NP_C_AMBIGUOUS, 0, 4 * 8, s));
        GHIP(hipMemsetAsync(P->mult.p, 0, n_rows * 4, s));
        ea.om = om; ea.row_of_entry = P->row_of_entry.as<u32>(); ea.mult = P->mult.as<u32>();
        hipLaunchKernelGGL(entry_kernel<true>, dim3(grid_for(ea.N)), dim3(256), 0, s, ea);
    } else
        hipLaunchKernelGGL(entry_kernel<false>, dim3(grid_for(ea.N)), dim3(256), 0, s, ea);
    if (R) {
        const RecordKeyArgs rk{ul.n_unitigs, R, ul.offsets, ul.edges.n1, ul.edges.o1, ul.edges.n2, ul.edges.o2, P->rkey.as<u64>(), P->rec.as<u32>(), counters};
        hipLaunchKernelGGL(record_key_kernel, dim3(grid_for(R)), dim3(256), 0, s, rk);
        GHIP(hipGetLastError());
        GHIP(sort_pairs(P->tmp, (const u64*)rk.rkey, P->rkey_sorted.as<u64>(), (const u32*)rk.rec, P->rec_sorted.as<u32>(), (size_t)R, 0u, 64u, s));
    }
    const ReadPathPlan plan{ea.entry_of_row, n_rows, ul.ori, P->code.as<u32>(), counters, ea.mult};
    placer.place(placer.ctx, plan, s);
    if (copies && n_idx) {
        u32* anchor = P->anchor.as<u32>(); u32* scanned = P->anchor_scan.as<u32>();
        const ResolveArgs ra{ul.n_entries, n_rows, n_idx, rg.i0, ul.offsets, ul.ori, ea.unitig_of_entry, ea.row_of_entry, rg.roff, rg.mread,
                             plan.code, anchor, anchor + n_idx, scanned, scanned + n_idx, counters};
        hipLaunchKernelGGL(mark_kernel, dim3(grid_for(n_idx)), dim3(256), 0, s, ra);
        GHIP(hipGetLastError());
        size_t tb = P->scan_tmp;               // (placement_reserve has asked for this range and grown tmp for it)
        if (P->scan_n != n_idx || tb > P->tmp.cap) return hipErrorInvalidValue;
        GHIP(rocprim::inclusive_scan(P->tmp.p, tb, (const u32*)ra.fwd, scanned, (size_t)n_idx, rocprim::maximum<u32>(), s));
        GHIP(rocprim::inclusive_scan(P->tmp.p, tb, (const u32*)ra.bwd, scanned + n_idx, (size_t)n_idx, rocprim::maximum<u32>(), s));
        hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(n_idx)), dim3(256), 0, s, ra);
    }
    *view = PlacementView{ea.entry_of_row, ea.unitig_of_entry, plan.code, counters, P->rkey_sorted.as<u64>(), P->rec_sorted.as<u32>(), R};
    return hipGetLastError();
}
