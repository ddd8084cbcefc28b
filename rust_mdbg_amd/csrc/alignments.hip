// alignments.hip — the steps of the read paths chained into alignments with base coordinates, on the GPU (gfx950).  Definition: include/mdbg_align.h
// (mdbg_graph_alignments).  Input: the device arrays of a unitig list (unitigs.hip) with its edge records, three columns of the node table (index, src_start, src_end), the
// store's read offsets, minimizer -> read map and raw positions, the placement with records (placement.h) and the read-path stage's steps (read_paths.h), which
// this call queues itself and whose kernels it shares: the step columns stay in the read-path unit's buffers.
//
//   (memset)            head2, the per-alignment sums and aln_step_offsets[0] <- 0
//   (read_paths_queue)  the placement with records, head_kernel, the scan, steps_kernel, finish_kernel, reads_kernel: the steps, flag[t] = 1 iff index t starts
//                       step pos[t]
//   chain_kernel        one thread per minimizer index t; the one that starts a step p (flag[t]) decides for it: the pair code[t - 1] -> code[t] is classified as in
//                       the junction and transit stages (classify_pair, placement_dev.h); an explained crossing chains p to p - 1 (the step in front ends at t - 1
//                       because t is a head and t - 1 is placed in the same read) and step_record[p] = the first record of the key's run; head2[p] = 1 iff p is not
//                       chained; step_index[p] = t.  n_chained is reduced per workgroup: one atomic
//   (rocPRIM)           apos = exclusive scan of head2 over n_idx + 1: step p belongs to alignment apos[p] + head2[p] - 1, and apos[n_steps] is their number
//   step_kernel         one thread per step: its wraps from first_entry, step_windows, strand and m(u) (the closing record of a ring by binary search); integer atomics
//                       add its windows and (1 + wraps) * length[u] minus its overlaps to its alignment; a head writes aln_step_offsets; the last step closes the list
//   aln_kernel          one thread per alignment: the query coordinates from the positions at its first and last window, path_begin and path_end from the pieces of
//                       its first and last entry (the entry's row by binary search in the table's index column)
//   aln_reads_kernel    one thread per read: aln_offsets[q] = apos[step_offsets[q]] (a read's first step starts an alignment)
//
// All sums are integers and every position comes from a sort or a scan: two calls give identical arrays.  No loop but the binary searches, no thread walks a run;
// the number of launches is fixed.  Per minimizer index of the range, beside the placement's 4 and the read paths' 5 + 17: 9 bytes of temporaries (head2 1, apos 4,
// step_index 4), 4 of step_record and 44 of alignment columns (aln_step_offsets 8, windows 4, query 8, path 24), sized for the worst case (every window a step and
// an alignment of its own) because their number is known only on the device.  Per read 8 (aln_offsets).  Per edge record the placement's 24.
#include <cstring>

#include "alignments.h"
#include "placement_dev.h"

struct AlignmentBuffers {
    Buf head2, apos, step_index, tmp;
    Buf aln_offsets, aln_step_offsets, step_record, aln_windows, query_begin, query_end, path_length, path_begin, path_end;      // the result
    StageTimer timer;
};

namespace {

struct AlArgs {
    u64 U, N, R, n_rows; const u64* offsets; const u8* circ; const u64* length; const u64* dst_offset; const u32* len; const u32* node; const u32* rec_overlap;
    const u32* index; const u64* src_start; const u64* src_end; const u32* positions; u32 l;
    const u32* unitig_of_entry; const u64* rkey_sorted; const u32* rec_sorted;
    const u64* roff; const u32* mread; u32 nr, k; u64 i0, n_idx;
    const u32* code; const u8* flag; const u32* pos; u64* counters;
    const u64* step_offsets; const u32* first_window; const u32* step_windows; const u32* unitig; const u32* first_entry; const u8* strand;
    u8* head2; const u32* apos; u32* step_index;
    u64* aln_offsets; u64* aln_step_offsets; u32* step_record; u32* aln_windows; u32* query_begin; u32* query_end; u64* path_length; u64* path_begin; u64* path_end;
};

__global__ __launch_bounds__(256) void chain_kernel(AlArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[1] = {0};
    if (t < a.n_idx && a.flag[t]) {
        const u32 p = a.pos[t];                            // (p < n_idx: a step per head)
        u64 key = 0, at = 0;
        u32 rec = RP_NONE;
        if (classify_pair(a.code, a.roff, a.mread, a.i0, t, a.code[t], a.unitig_of_entry, a.rkey_sorted, a.R, &key, &at) == PAIR_EXPLAINED) {
            rec = a.rec_sorted[at];
            if (rec >= a.R) { set_defect(a.counters, AL_DEFECT_RECORD); rec = RP_NONE; }
        }
        a.step_record[p] = rec; a.step_index[p] = (u32)t; a.head2[p] = rec == RP_NONE;
        cnt[0] = rec != RP_NONE;
    }
    block_add<1>(cnt, a.counters, AL_C_CHAINED);
}

// the bases two consecutive occurrences of a path share over record r: a record's overlap is counted on the reference's seqlen, last position + 1 - first position + 1
// (src/main.rs:778), which is l - 2 short of the node's sequence (first position .. last position + l)
__device__ inline u64 base_overlap(const AlArgs& a, u32 r) { return (u64)a.rec_overlap[r] + a.l - 2; }
// the ring closures inside a step of n windows that starts at entry j of a unitig of m entries
__device__ inline u64 wraps_of(bool circular, u64 m, u64 j, u64 n, u32 s) { return circular ? ((s ? m - 1 - j : j) + n - 1) / m : 0; }

__global__ __launch_bounds__(256) void step_kernel(AlArgs a) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 n_steps = a.counters[RP_C_STEPS];            // (the grid is sized for one step per index)
    u32 cnt[1] = {0};
    if (p < n_steps) {
        const u32 u = a.unitig[p], n = a.step_windows[p], s = a.strand[p], h = a.head2[p];
        const u64 first = a.offsets[u], m = a.offsets[u + 1] - first;
        const u64 w = wraps_of(a.circ[u] != 0, m, a.first_entry[p], n, s);
        u64 overlaps = 0;
        if (w) {                                           // the closing record u + u +: the smallest record with the wrap's key
            const u64 key = key_of_pair((u32)((first + m - 1) << 1), (u32)(first << 1));
            const u64 at = lower_bound(a.rkey_sorted, a.R, key);
            const u32 r = at < a.R && a.rkey_sorted[at] == key ? a.rec_sorted[at] : RP_NONE;
            if (r < a.R) overlaps = w * base_overlap(a, r); else set_defect(a.counters, AL_DEFECT_RECORD);
        }
        if (!h) {
            const u32 r = a.step_record[p];
            if (r < a.R) overlaps += base_overlap(a, r); else set_defect(a.counters, AL_DEFECT_RECORD);
        }
        const u32 A = a.apos[p] + h - 1;                   // (step 0 is a head: apos + h >= 1)
        atomicAdd(a.aln_windows + A, n);
        atomicAdd((unsigned long long*)(a.path_length + A), (unsigned long long)((1 + w) * a.length[u] - overlaps));      // (modulo 2^64: the alignment's sum is what counts)
        if (h) a.aln_step_offsets[A] = p;
        if (p + 1 == n_steps) { a.aln_step_offsets[A + 1] = n_steps; a.counters[AL_C_ALIGNMENTS] = (u64)A + 1; }
        cnt[0] = (u32)w;
    }
    block_add<1>(cnt, a.counters, AL_C_WRAPS);
}

// the piece of the unitig's sequence the node of global entry e covers: [*b, *e_) with E = dst_offset + len, B = E - (src_end - src_start)[row], clamped at 0.  false: no row
__device__ inline bool span_of_entry(const AlArgs& a, u64 e, u64* b, u64* e_) {
    const u32 idx = a.node[e];
    u64 lo = 0, hi = a.n_rows;                             // as entry_kernel (placement.hip): rows are in index order
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.index[mid] < idx) lo = mid + 1; else hi = mid; }
    if (lo >= a.n_rows || a.index[lo] != idx) return false;
    const u64 E = a.dst_offset[e] + a.len[e], sl = a.src_end[lo] - a.src_start[lo];
    *e_ = E; *b = E > sl ? E - sl : 0;
    return true;
}

__global__ __launch_bounds__(256) void aln_kernel(AlArgs a) {
    const u64 A = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (A >= a.counters[AL_C_ALIGNMENTS]) return;          // (the grid is sized for one alignment per index)
    const u64 p0 = a.aln_step_offsets[A], p1 = a.aln_step_offsets[A + 1] - 1;
    const u64 t0 = a.step_index[p0], t1 = (u64)a.step_index[p1] + a.step_windows[p1] - 1;      // the indices of the first and the last window
    if (t1 + a.k - 1 >= a.n_idx) { set_defect(a.counters, AL_DEFECT_RECORD); return; }
    a.query_begin[A] = a.positions[a.i0 + t0];
    a.query_end[A] = a.positions[a.i0 + t1 + a.k - 1] + a.l;                                   // src/main.rs:778
    const u32 u0 = a.unitig[p0], s0 = a.strand[p0], u1 = a.unitig[p1], s1 = a.strand[p1];
    const u64 f1 = a.offsets[u1], m1 = a.offsets[u1 + 1] - f1, d1 = ((u64)a.step_windows[p1] - 1) % m1, j1 = a.first_entry[p1];
    const u64 last = s1 ? (j1 + m1 - d1) % m1 : (j1 + d1) % m1;                                // the last window's entry (a linear unitig never gets to the modulo)
    u64 b0, e0, b1, e1;
    if (!span_of_entry(a, a.offsets[u0] + a.first_entry[p0], &b0, &e0) || !span_of_entry(a, f1 + last, &b1, &e1)) { set_defect(a.counters, RP_DEFECT_ENTRY); return; }
    a.path_begin[A] = s0 ? a.length[u0] - e0 : b0;
    a.path_end[A] = a.path_length[A] - (s1 ? b1 : a.length[u1] - e1);
}

__global__ __launch_bounds__(256) void aln_reads_kernel(AlArgs a) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > a.nr) return;
    a.aln_offsets[q] = a.n_idx ? (u64)a.apos[a.step_offsets[q]] : 0;     // (step_offsets <= n_steps <= n_idx: inside the n_idx + 1 scanned)
}

}  // namespace

AlignmentBuffers* alignment_buffers_create() { return new AlignmentBuffers(); }
void alignment_buffers_destroy(AlignmentBuffers* b) { delete b; }

hipError_t alignments_run(AlignmentBuffers* A, ReadPathBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const AlignmentNodes& nd, const ReadPathRange& rg,
                          const WindowPlacer& placer, hipStream_t s, ReadPathResult* rp, AlignmentResult* out) {
    memset(out, 0, sizeof *out); memset(rp, 0, sizeof *rp);
    const u64 n_idx = rg.i1 - rg.i0, nr = rg.n_reads;
    // every buffer first: growing one may wait for the device (graph_common.h), and nothing of this call is queued yet
    GHIP(read_paths_reserve(B, P, ul, nd.n_rows, rg, true));
    GHIP(A->head2.ensure(n_idx + 4)); GHIP(A->apos.ensure(n_idx * 4 + 8)); GHIP(A->step_index.ensure(n_idx * 4 + 4)); GHIP(A->step_record.ensure(n_idx * 4 + 4));
    GHIP(A->aln_offsets.ensure((nr + 1) * 8)); GHIP(A->aln_step_offsets.ensure((n_idx + 1) * 8));
    GHIP(A->aln_windows.ensure(n_idx * 4 + 4)); GHIP(A->query_begin.ensure(n_idx * 4 + 4)); GHIP(A->query_end.ensure(n_idx * 4 + 4));
    GHIP(A->path_length.ensure(n_idx * 8 + 8)); GHIP(A->path_begin.ensure(n_idx * 8 + 8)); GHIP(A->path_end.ensure(n_idx * 8 + 8));
    if (n_idx) { size_t tb = 0; GHIP(rocprim::exclusive_scan(nullptr, tb, A->head2.as<u8>(), A->apos.as<u32>(), 0u, (size_t)n_idx + 1, rocprim::plus<u32>(), hipStream_t(nullptr))); GHIP(A->tmp.ensure(tb + 256)); }
    GHIP(A->timer.start(s));
    GHIP(hipMemsetAsync(A->head2.p, 0, n_idx + 1, s)); GHIP(hipMemsetAsync(A->aln_windows.p, 0, n_idx * 4 + 4, s)); GHIP(hipMemsetAsync(A->path_length.p, 0, n_idx * 8 + 8, s));
    GHIP(hipMemsetAsync(A->aln_step_offsets.p, 0, 8, s));
    PlacementView V; ReadPathScratch sc{};
    GHIP(read_paths_queue(B, P, ul, nd.index, nd.n_rows, rg, true, AL_C_N, placer, s, &V, rp, &sc));
    AlArgs a; memset(&a, 0, sizeof a);
    a.U = ul.n_unitigs; a.N = ul.n_entries; a.R = V.R; a.n_rows = nd.n_rows; a.offsets = ul.offsets; a.circ = ul.circular; a.length = ul.length; a.dst_offset = ul.dst_offset; a.len = ul.len;
    a.node = ul.node; a.rec_overlap = ul.edges.overlap; a.index = nd.index; a.src_start = nd.src_start; a.src_end = nd.src_end; a.positions = nd.positions; a.l = nd.l;
    a.unitig_of_entry = V.unitig_of_entry; a.rkey_sorted = V.rkey_sorted; a.rec_sorted = V.rec_sorted;
    a.roff = rg.roff; a.mread = rg.mread; a.nr = rg.n_reads; a.k = rg.k; a.i0 = rg.i0; a.n_idx = n_idx;
    a.code = V.code; a.flag = sc.flag; a.pos = sc.pos; a.counters = V.counters;
    a.step_offsets = rp->step_offsets; a.first_window = rp->first_window; a.step_windows = rp->step_windows; a.unitig = rp->unitig; a.first_entry = rp->first_entry; a.strand = rp->strand;
    a.head2 = A->head2.as<u8>(); a.apos = A->apos.as<u32>(); a.step_index = A->step_index.as<u32>();
    a.aln_offsets = A->aln_offsets.as<u64>(); a.aln_step_offsets = A->aln_step_offsets.as<u64>(); a.step_record = A->step_record.as<u32>(); a.aln_windows = A->aln_windows.as<u32>();
    a.query_begin = A->query_begin.as<u32>(); a.query_end = A->query_end.as<u32>(); a.path_length = A->path_length.as<u64>(); a.path_begin = A->path_begin.as<u64>(); a.path_end = A->path_end.as<u64>();
    if (n_idx) {
        const unsigned gi = grid_for(n_idx);
        hipLaunchKernelGGL(chain_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(hipGetLastError());
        GHIP(excl_scan(A->tmp, (const u8*)a.head2, A->apos.as<u32>(), (size_t)n_idx + 1, s));
        hipLaunchKernelGGL(step_kernel, dim3(gi), dim3(256), 0, s, a);
        hipLaunchKernelGGL(aln_kernel, dim3(gi), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(aln_reads_kernel, dim3(grid_for(nr + 1)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    u64 h[AL_C_N];
    GHIP(A->timer.stop_and_read(h, a.counters, sizeof h, s, &out->ms));
    read_paths_counts(h, rp);
    rp->ms = out->ms;
    out->defect = rp->defect;
    if (out->defect) { const u32 d = out->defect; const float ms = out->ms; memset(rp, 0, sizeof *rp); memset(out, 0, sizeof *out); rp->defect = out->defect = d; rp->ms = out->ms = ms; return hipSuccess; }
    out->n_chained = h[AL_C_CHAINED]; out->n_alignments = h[AL_C_ALIGNMENTS]; out->n_wraps = h[AL_C_WRAPS];
    out->aln_offsets = a.aln_offsets; out->aln_step_offsets = a.aln_step_offsets; out->step_record = a.step_record; out->aln_windows = a.aln_windows;
    out->query_begin = a.query_begin; out->query_end = a.query_end; out->path_length = a.path_length; out->path_begin = a.path_begin; out->path_end = a.path_end;
    return hipSuccess;
}
