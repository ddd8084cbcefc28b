// read_paths.hip — the resident reads threaded through the current unitig list, on the GPU (gfx950): everything of the stage behind the placement.
// Definition: include/mdbg_hip.h (mdbg_graph_read_paths).  Input: the device arrays of a unitig list (unitigs.hip), the store's read offsets and minimizer ->
// read map, and the placement (placement.h): unitig_of_entry and the per-index codes, in the context's one placement scratch.
//
//   (memset)            the support sums <- 0
//   (placement_queue)   the counters and the map zeroed, entry_kernel, place_windows_kernel: code[t] = entry | strand << 31 of the window that starts at index
//                       i0 + t, or NONE
//   head_kernel         flag[t] = 1 iff code[t] is a window and does not continue code[t - 1] inside the same read (same unitig and strand, the entry
//                       one further in the read's direction, modulo the size on a circular unitig)
//   (rocPRIM)           pos = exclusive scan of flag: a window's step is pos + flag - 1, the range's steps are numbered in index order
//   steps_kernel        a head writes its step's first_window, unitig, first_entry, strand; the LAST window of a run (the next code is NONE, a head, or
//                       the range ends) writes its window number + 1 into step_windows — the p-th head and the p-th run end belong to one step, so
//                       nobody walks a run
//   finish_kernel       one thread per step: step_windows -= first_window; integer atomics add the step to its unitig's two sums
//   reads_kernel        one thread per read: step_offsets[q] = pos at the read's first index, ordinal[q] from the batch table, read_windows[q] from its offsets
//
// All sums are integers and every position comes from the scan: two calls give identical arrays.  No loop but the binary search of reads_kernel; the number of
// launches is fixed.  Per minimizer index of the range, beside the placement's 4: 5 bytes of temporaries (flag 1, pos 4) and 17 of step columns, sized for the
// worst case (every window a step of its own).
#include <cstring>

#include "read_paths.h"
#include "placement_dev.h"

struct ReadPathBuffers {
    Buf flag, pos, tmp;
    Buf ordinal, read_windows, step_offsets, first_window, step_windows, unitig, first_entry, strand, sup_w, sup_s;      // the result
    StageTimer timer;
};

namespace {

struct RpArgs {
    u64 U; const u64* offsets; const u8* circ; const u32* unitig_of_entry;
    const u64* roff; const u32* mread; u32 r0, nr, k; u64 i0, n_idx;
    const u32* code; u8* flag; const u32* pos; u64* counters;
    u64* ordinal; u32* read_windows; u64* step_offsets; u32* first_window; u32* step_windows; u32* unitig; u32* first_entry; u8* strand; u64* sup_w; u64* sup_s;
    const u32* by_slot0; const u64* by_slot_first; u32 n_batches;
};

// does the placed window with code c continue the placed window with code pc (the index in front of it, same read)?
__device__ inline bool continues(const RpArgs& a, u32 pc, u32 c) {
    if ((pc ^ c) & RP_STRAND) return false;
    const u32 e = c & ~RP_STRAND, pe = pc & ~RP_STRAND;
    const u32 u = a.unitig_of_entry[e];
    if (a.unitig_of_entry[pe] != u) return false;
    const u64 first = a.offsets[u], last = a.offsets[u + 1] - 1;
    const bool circ = a.circ[u] != 0;
    if (!(c & RP_STRAND)) return e == pe + 1 || (circ && pe == last && e == first);
    return pe == e + 1 || (circ && pe == first && e == last);
}

__global__ __launch_bounds__(256) void head_kernel(RpArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u32 c = a.code[t];
    u8 f = 0;
    if (c != RP_NONE) {
        u32 pc;
        f = !(adjacent_in_read(a.code, a.roff, a.mread, a.i0, t, c, &pc) && continues(a, pc, c));
    }
    a.flag[t] = f;
}

__global__ __launch_bounds__(256) void steps_kernel(RpArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u32 f = a.flag[t], before = a.pos[t];
    if (t == a.n_idx - 1) a.counters[RP_C_STEPS] = (u64)before + f;
    const u32 c = a.code[t];
    if (c == RP_NONE) return;
    const u32 p = before + f - 1;                          // (a window that is no head has a head in front of it: before >= 1)
    const u64 i = a.i0 + t;
    const u32 w = (u32)(i - a.roff[a.mread[i]]);
    if (f) {
        const u32 e = c & ~RP_STRAND, u = a.unitig_of_entry[e];
        a.first_window[p] = w; a.unitig[p] = u; a.first_entry[p] = (u32)(e - a.offsets[u]); a.strand[p] = (u8)(c >> 31);
    }
    const bool last = t + 1 == a.n_idx || a.code[t + 1] == RP_NONE || a.flag[t + 1] != 0;      // (a read's first window is a head or no window)
    if (last) a.step_windows[p] = w + 1;
}

__global__ __launch_bounds__(256) void finish_kernel(RpArgs a) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.counters[RP_C_STEPS]) return;               // (the grid is sized for one step per index)
    const u32 n = a.step_windows[p] - a.first_window[p];
    a.step_windows[p] = n;
    const u32 u = a.unitig[p];
    atomicAdd((unsigned long long*)(a.sup_s + u), 1ull);
    atomicAdd((unsigned long long*)(a.sup_w + u), (unsigned long long)n);
}

__global__ __launch_bounds__(256) void reads_kernel(RpArgs a) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > a.nr) return;
    const u64 t = a.roff[a.r0 + q] - a.i0;
    a.step_offsets[q] = t < a.n_idx ? (u64)a.pos[t] : a.n_idx ? (u64)a.pos[a.n_idx - 1] + a.flag[a.n_idx - 1] : 0;
    if (q == a.nr) return;
    const u64 n_min = a.roff[a.r0 + q + 1] - a.roff[a.r0 + q];
    a.read_windows[q] = n_min > a.k ? (u32)(n_min - a.k + 1) : 0u;      // src/main.rs:756-759
    if (a.n_batches == 0) { a.ordinal[q] = q; return; }   // a range without a batch table (a temporary batch, mdbg_graph_align_batch): the read's number in the range
    const u32 slot = a.r0 + (u32)q;
    u32 lo = 0, hi = a.n_batches - 1;                      // as rep_ordinal (finalize.hip): the last batch whose first slot is <= slot
    while (lo < hi) { const u32 mid = lo + ((hi - lo + 1) >> 1); if (a.by_slot0[mid] <= slot) lo = mid; else hi = mid - 1; }
    a.ordinal[q] = a.by_slot_first[lo] + (slot - a.by_slot0[lo]);
}

RpArgs args_of(ReadPathBuffers* B, const PlacementView& V, const UnitigResult& ul, const ReadPathRange& rg) {
    RpArgs a; memset(&a, 0, sizeof a);
    a.U = ul.n_unitigs; a.offsets = ul.offsets; a.circ = ul.circular; a.unitig_of_entry = V.unitig_of_entry;
    a.roff = rg.roff; a.mread = rg.mread; a.r0 = rg.first_read; a.nr = rg.n_reads; a.k = rg.k; a.i0 = rg.i0; a.n_idx = rg.i1 - rg.i0;
    a.code = V.code; a.flag = B->flag.as<u8>(); a.pos = B->pos.as<u32>(); a.counters = V.counters;
    a.ordinal = B->ordinal.as<u64>(); a.read_windows = B->read_windows.as<u32>(); a.step_offsets = B->step_offsets.as<u64>(); a.first_window = B->first_window.as<u32>(); a.step_windows = B->step_windows.as<u32>();
    a.unitig = B->unitig.as<u32>(); a.first_entry = B->first_entry.as<u32>(); a.strand = B->strand.as<u8>(); a.sup_w = B->sup_w.as<u64>(); a.sup_s = B->sup_s.as<u64>();
    a.by_slot0 = rg.by_slot0; a.by_slot_first = rg.by_slot_first; a.n_batches = rg.n_batches;
    return a;
}

}  // namespace

ReadPathBuffers* read_path_buffers_create() { return new ReadPathBuffers(); }
void read_path_buffers_destroy(ReadPathBuffers* b) { delete b; }

hipError_t read_paths_reserve(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, u64 n_rows, const ReadPathRange& rg, bool with_records) {
    const u64 U = ul.n_unitigs, n_idx = rg.i1 - rg.i0, nr = rg.n_reads;
    GHIP(placement_reserve(P, ul, n_rows, rg, with_records));
    GHIP(B->flag.ensure(n_idx + 4)); GHIP(B->pos.ensure(n_idx * 4 + 4));
    GHIP(B->ordinal.ensure(nr * 8 + 8)); GHIP(B->read_windows.ensure(nr * 4 + 4)); GHIP(B->step_offsets.ensure((nr + 1) * 8));
    GHIP(B->first_window.ensure(n_idx * 4 + 4)); GHIP(B->step_windows.ensure(n_idx * 4 + 4)); GHIP(B->unitig.ensure(n_idx * 4 + 4)); GHIP(B->first_entry.ensure(n_idx * 4 + 4));
    GHIP(B->strand.ensure(n_idx + 4)); GHIP(B->sup_w.ensure(U * 8)); GHIP(B->sup_s.ensure(U * 8));
    if (n_idx) { size_t tb = 0; GHIP(rocprim::exclusive_scan(nullptr, tb, B->flag.as<u8>(), B->pos.as<u32>(), 0u, (size_t)n_idx, rocprim::plus<u32>(), hipStream_t(nullptr))); GHIP(B->tmp.ensure(tb + 256)); }
    return hipSuccess;
}

hipError_t read_paths_queue(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const u32* index, u64 n_rows, const ReadPathRange& rg, bool with_records, u32 n_counters,
                            const WindowPlacer& placer, hipStream_t s, PlacementView* V, ReadPathResult* out, ReadPathScratch* scratch) {
    memset(out, 0, sizeof *out);
    const u64 U = ul.n_unitigs;
    GHIP(hipMemsetAsync(B->sup_w.p, 0, U * 8, s)); GHIP(hipMemsetAsync(B->sup_s.p, 0, U * 8, s));
    GHIP(placement_queue(P, ul, index, n_rows, rg, with_records, n_counters, placer, s, V));
    const RpArgs a = args_of(B, *V, ul, rg);
    if (a.n_idx) {
        const unsigned gi = grid_for(a.n_idx);
        hipLaunchKernelGGL(head_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(excl_scan(B->tmp, B->flag.as<u8>(), B->pos.as<u32>(), (size_t)a.n_idx, s));
        hipLaunchKernelGGL(steps_kernel, dim3(gi), dim3(256), 0, s, a);
        hipLaunchKernelGGL(finish_kernel, dim3(gi), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(reads_kernel, dim3(grid_for((u64)a.nr + 1)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    out->n_reads = a.nr; out->n_unitigs = a.U;
    out->ordinal = a.ordinal; out->read_windows = a.read_windows; out->step_offsets = a.step_offsets; out->first_window = a.first_window; out->step_windows = a.step_windows; out->unitig = a.unitig;
    out->first_entry = a.first_entry; out->strand = a.strand; out->support_windows = a.sup_w; out->support_steps = a.sup_s;
    if (scratch) { scratch->flag = a.flag; scratch->pos = a.pos; }
    return hipSuccess;
}

void read_paths_counts(const u64* h, ReadPathResult* out) {
    out->defect = (u32)h[RP_C_DEFECT];
    out->n_windows = h[RP_C_WINDOWS]; out->n_placed = h[RP_C_PLACED]; out->n_steps = h[RP_C_STEPS];
}

hipError_t read_paths_run(ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const u32* index, u64 n_rows, const ReadPathRange& rg, const WindowPlacer& placer,
                          hipStream_t s, ReadPathResult* out) {
    memset(out, 0, sizeof *out);
    // every buffer first: growing one may wait for the device (graph_common.h), and nothing of this call is queued yet
    GHIP(read_paths_reserve(B, P, ul, n_rows, rg, false));
    GHIP(B->timer.start(s));
    PlacementView V;
    GHIP(read_paths_queue(B, P, ul, index, n_rows, rg, false, RP_C_N, placer, s, &V, out, nullptr));
    u64 h[RP_C_N];
    float ms = 0;
    GHIP(B->timer.stop_and_read(h, V.counters, sizeof h, s, &ms));
    read_paths_counts(h, out);
    out->ms = ms;
    if (out->defect) { const u32 d = out->defect; memset(out, 0, sizeof *out); out->defect = d; out->ms = ms; }
    return hipSuccess;
}
