// chains.hip — consecutive alignments of one read joined over a BRIDGE into chains, on the GPU (gfx950).  Definition: include/mdbg_chain.h (mdbg_graph_chains).
// Input, all on the device behind alignments_run of the same range: the steps (read_paths.h), the alignments (alignments.h), the list's offsets, lengths and record
// overlaps (unitigs.hip) and the record keys the placement has sorted (placement_records).  The host knows n_alignments from that call's one wait, so every buffer and
// grid here is sized by it, not by the minimizer indices.
//
//   (memset)            five: the counters, the ONE byte head[n_alignments] behind the flags bridge_kernel writes (the scan runs over n_alignments + 1), and the three
//                       per-chain sums (windows, gap windows, path length) <- 0
//   bridge_kernel       one thread per alignment a: the first of a read (its read by binary search in aln_offsets) is a head; any other takes the last step of a - 1
//                       and its own first step, builds the INSIDE and the RECORD candidate (one lower_bound in the sorted record keys), takes the nearer one and
//                       applies the thresholds: bridge_record, bridge_entries, head[a] = 1 iff not bridged, and for chain_sum_kernel the bases the bridge takes off the path
//                       and its gap windows.  The three counters are reduced per workgroup: one atomic each
//   (rocPRIM)           cpos = exclusive scan of head over n_alignments + 1: alignment a belongs to chain cpos[a] + head[a] - 1
//   chain_sum_kernel    one thread per alignment: integer atomics add its windows, its gap windows and its path length minus what its bridge takes off to its chain;
//                       a head writes chain_aln_offsets; the last alignment closes the list and leaves the number of chains
//   chain_coord_kernel  one thread per chain: the query and path coordinates from its first and its last alignment
//   chain_reads_kernel  one thread per read: chain_offsets[q] = cpos[aln_offsets[q]] (a read's first alignment starts a chain)
//
// All sums are integers and every position comes from a scan: two calls give identical arrays.  No loop but the binary searches; the number of launches is fixed.
// Per alignment 17 bytes of temporaries (head 1, cpos 4, cut 8, gap 4), 12 of bridge columns and 48 of chain columns; per read 8 (chain_offsets).
#include <cstring>

#include "chains.h"
#include "placement_dev.h"

struct ChainBuffers {
    Buf head, cpos, cut, gap, counters, tmp;
    Buf bridge_record, bridge_entries, chain_offsets, chain_aln_offsets, chain_windows, chain_gap_windows, query_begin, query_end, path_length, path_begin, path_end;      // the result
    StageTimer timer;
};

namespace {

// counters[]: the defect mask sits where set_defect (placement_dev.h) writes it
enum { CH_C_INSIDE = 0, CH_C_RECORD, CH_C_GAP, CH_C_DEFECT = RP_C_DEFECT, CH_C_CHAINS, CH_C_N };
static_assert(CH_C_GAP < CH_C_DEFECT, "block_add<3> ends in front of the defect mask");

struct ChArgs {
    u64 na, nr, n_steps, U, R; u32 l, max_skew, max_gap;
    const u64* offsets; const u64* length; const u32* rec_overlap; const u64* rkey_sorted; const u32* rec_sorted;
    const u32* first_window; const u32* step_windows; const u32* unitig; const u32* first_entry; const u8* strand;
    const u64* aln_offsets; const u64* aln_step_offsets; const u32* aln_windows; const u32* aq_begin; const u32* aq_end; const u64* a_plen; const u64* a_pbeg; const u64* a_pend;
    u8* head; const u32* cpos; u64* cut; u32* gap; u64* counters;
    u32* bridge_record; u64* bridge_entries; u64* chain_offsets; u64* chain_aln_offsets; u32* chain_windows; u32* chain_gap_windows; u32* query_begin; u32* query_end;
    u64* path_length; u64* path_begin; u64* path_end;
};

__device__ inline u64 abs_diff(u64 a, u64 b) { return a > b ? a - b : b - a; }

__global__ __launch_bounds__(256) void bridge_kernel(ChArgs a) {
    const u64 A = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[3] = {0, 0, 0};            // inside, record, gap windows
    if (A < a.na) {
        u32 rec = RP_NONE; u64 entries = 0, cut = 0; u32 gap = 0;
        bool same_read = false;
        if (A) {                       // the read of A: the last q with aln_offsets[q] <= A; A is its first alignment iff the two are equal
            u64 lo = 0, hi = a.nr;
            while (lo < hi) { const u64 mid = lo + ((hi - lo + 1) >> 1); if (a.aln_offsets[mid] <= A) lo = mid; else hi = mid - 1; }
            same_read = a.aln_offsets[lo] != A;
        }
        const u64 py = same_read ? a.aln_step_offsets[A] : 0;
        if (same_read && (py == 0 || py >= a.n_steps)) { set_defect(a.counters, AL_DEFECT_RECORD); same_read = false; }
        if (same_read) {
            const u64 px = py - 1;
            const u32 ux = a.unitig[px], uy = a.unitig[py], sx = a.strand[px] != 0, sy = a.strand[py] != 0, nx = a.step_windows[px];
            if (ux >= a.U || uy >= a.U || nx == 0) set_defect(a.counters, AL_DEFECT_RECORD);
            else {
                const u64 fx = a.offsets[ux], mx = a.offsets[ux + 1] - fx, fy = a.offsets[uy], my = a.offsets[uy + 1] - fy;
                const u64 j0 = a.first_entry[px], jy = a.first_entry[py];
                const u64 wx = (u64)a.first_window[px] + nx - 1, wy = a.first_window[py];
                if (mx == 0 || my == 0 || j0 >= mx || jy >= my || wy <= wx) set_defect(a.counters, AL_DEFECT_RECORD);
                else {
                    const u64 d = ((u64)nx - 1) % mx, jx = sx ? (j0 + mx - d) % mx : (j0 + d) % mx;      // the last window's entry, as aln_kernel (alignments.hip) has it
                    const u64 dw = wy - wx;
                    // INSIDE: the same unitig and strand, further on in walk direction (no modulo)
                    const bool in_ok = ux == uy && sx == sy && (sx ? jx > jy : jy > jx);
                    const u64 in_e = in_ok ? (sx ? jx - jy : jy - jx) : 0;
                    // RECORD: from the last vertex of u_x in direction s_x to the first of u_y in direction s_y
                    const u64 key = key_of_pair((u32)((fx + (sx ? 0 : mx - 1)) << 1) | sx, (u32)((fy + (sy ? my - 1 : 0)) << 1) | sy);
                    const u64 at = lower_bound(a.rkey_sorted, a.R, key);
                    u32 r = at < a.R && a.rkey_sorted[at] == key ? a.rec_sorted[at] : RP_NONE;
                    if (r != RP_NONE && r >= a.R) { set_defect(a.counters, AL_DEFECT_RECORD); r = RP_NONE; }
                    const u64 rec_e = (sx ? jx : mx - 1 - jx) + (sy ? my - 1 - jy : jy) + 1;
                    const bool inside = in_ok && (r == RP_NONE || abs_diff(in_e, dw) <= abs_diff(rec_e, dw));      // the nearer candidate first, a tie to INSIDE: then the thresholds
                    if (inside || r != RP_NONE) {
                        const u64 e = inside ? in_e : rec_e;
                        if (dw >= 2 && abs_diff(e, dw) <= a.max_skew && (a.max_gap == 0 || dw - 1 <= a.max_gap)) {
                            rec = inside ? CH_INSIDE : r; entries = e; gap = (u32)(dw - 1);
                            cut = inside ? a.length[ux] : (u64)a.rec_overlap[r] + a.l - 2;      // the occurrence the two share, or the record's base overlap
                            cnt[inside ? 0 : 1] = 1; cnt[2] = gap;
                        }
                    }
                }
            }
        }
        a.bridge_record[A] = rec; a.bridge_entries[A] = entries; a.cut[A] = cut; a.gap[A] = gap; a.head[A] = rec == RP_NONE;
    }
    block_add<3>(cnt, a.counters, CH_C_INSIDE);
}

__global__ __launch_bounds__(256) void chain_sum_kernel(ChArgs a) {
    const u64 A = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (A >= a.na) return;
    const u32 h = a.head[A];
    const u32 c = a.cpos[A] + h - 1;                       // (alignment 0 is a head: cpos + h >= 1; c < na)
    atomicAdd(a.chain_windows + c, a.aln_windows[A]);
    if (!h) atomicAdd(a.chain_gap_windows + c, a.gap[A]);
    atomicAdd((unsigned long long*)(a.path_length + c), (unsigned long long)(a.a_plen[A] - a.cut[A]));      // (modulo 2^64: the chain's sum is what counts)
    if (h) a.chain_aln_offsets[c] = A;
    if (A + 1 == a.na) { a.chain_aln_offsets[c + 1] = a.na; a.counters[CH_C_CHAINS] = (u64)c + 1; }
}

__global__ __launch_bounds__(256) void chain_coord_kernel(ChArgs a) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.na || c >= a.counters[CH_C_CHAINS]) return;      // (the grid is sized for one chain per alignment)
    const u64 a0 = a.chain_aln_offsets[c], a1 = a.chain_aln_offsets[c + 1] - 1;
    if (a0 >= a.na || a1 >= a.na) { set_defect(a.counters, AL_DEFECT_RECORD); return; }
    a.query_begin[c] = a.aq_begin[a0]; a.query_end[c] = a.aq_end[a1];
    a.path_begin[c] = a.a_pbeg[a0];
    a.path_end[c] = a.path_length[c] - (a.a_plen[a1] - a.a_pend[a1]);
}

__global__ __launch_bounds__(256) void chain_reads_kernel(ChArgs a) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > a.nr) return;
    const u64 A = a.aln_offsets[q];
    a.chain_offsets[q] = A <= a.na ? (u64)a.cpos[A] : 0;    // (cpos has n_alignments + 1 elements)
}

}  // namespace

ChainBuffers* chain_buffers_create() { return new ChainBuffers(); }
void chain_buffers_destroy(ChainBuffers* b) { delete b; }

hipError_t chains_run(ChainBuffers* C, const PlacementBuffers* P, const UnitigResult& ul, const ReadPathResult& rp, const AlignmentResult& al, u32 l, u32 max_skew, u32 max_gap,
                      hipStream_t s, ChainResult* out) {
    memset(out, 0, sizeof *out);
    const u64 na = al.n_alignments, nr = rp.n_reads;
    if (na == 0) {                                         // nothing to join: the two offset columns are zeros; no launch, no wait
        GHIP(C->chain_offsets.ensure((nr + 1) * 8)); GHIP(C->chain_aln_offsets.ensure(8));
        GHIP(hipMemsetAsync(C->chain_offsets.p, 0, (nr + 1) * 8, s)); GHIP(hipMemsetAsync(C->chain_aln_offsets.p, 0, 8, s));
        out->chain_offsets = C->chain_offsets.as<u64>(); out->chain_aln_offsets = C->chain_aln_offsets.as<u64>();
        return hipSuccess;
    }
    if (na >= 0xFFFFFFF0ull) return hipErrorInvalidValue;  // (alignments_run has bounded the minimizer indices, and there are fewer alignments)
    // every buffer first: growing one may wait for the device (graph_common.h), and nothing of this call is queued yet
    GHIP(C->counters.ensure(CH_C_N * 8));
    GHIP(C->head.ensure(na + 1)); GHIP(C->cpos.ensure(na * 4 + 4)); GHIP(C->cut.ensure(na * 8)); GHIP(C->gap.ensure(na * 4));
    GHIP(C->bridge_record.ensure(na * 4)); GHIP(C->bridge_entries.ensure(na * 8)); GHIP(C->chain_offsets.ensure((nr + 1) * 8)); GHIP(C->chain_aln_offsets.ensure((na + 1) * 8));
    GHIP(C->chain_windows.ensure(na * 4)); GHIP(C->chain_gap_windows.ensure(na * 4)); GHIP(C->query_begin.ensure(na * 4)); GHIP(C->query_end.ensure(na * 4));
    GHIP(C->path_length.ensure(na * 8)); GHIP(C->path_begin.ensure(na * 8)); GHIP(C->path_end.ensure(na * 8));
    { size_t tb = 0; GHIP(rocprim::exclusive_scan(nullptr, tb, C->head.as<u8>(), C->cpos.as<u32>(), 0u, (size_t)na + 1, rocprim::plus<u32>(), hipStream_t(nullptr))); GHIP(C->tmp.ensure(tb + 256)); }
    ChArgs a; memset(&a, 0, sizeof a);
    a.na = na; a.nr = nr; a.n_steps = rp.n_steps; a.U = ul.n_unitigs; a.R = ul.edges.n; a.l = l; a.max_skew = max_skew; a.max_gap = max_gap;
    a.offsets = ul.offsets; a.length = ul.length; a.rec_overlap = ul.edges.overlap;
    placement_records(P, &a.rkey_sorted, &a.rec_sorted);
    a.first_window = rp.first_window; a.step_windows = rp.step_windows; a.unitig = rp.unitig; a.first_entry = rp.first_entry; a.strand = rp.strand;
    a.aln_offsets = al.aln_offsets; a.aln_step_offsets = al.aln_step_offsets; a.aln_windows = al.aln_windows; a.aq_begin = al.query_begin; a.aq_end = al.query_end;
    a.a_plen = al.path_length; a.a_pbeg = al.path_begin; a.a_pend = al.path_end;
    a.head = C->head.as<u8>(); a.cpos = C->cpos.as<u32>(); a.cut = C->cut.as<u64>(); a.gap = C->gap.as<u32>(); a.counters = C->counters.as<u64>();
    a.bridge_record = C->bridge_record.as<u32>(); a.bridge_entries = C->bridge_entries.as<u64>(); a.chain_offsets = C->chain_offsets.as<u64>(); a.chain_aln_offsets = C->chain_aln_offsets.as<u64>();
    a.chain_windows = C->chain_windows.as<u32>(); a.chain_gap_windows = C->chain_gap_windows.as<u32>(); a.query_begin = C->query_begin.as<u32>(); a.query_end = C->query_end.as<u32>();
    a.path_length = C->path_length.as<u64>(); a.path_begin = C->path_begin.as<u64>(); a.path_end = C->path_end.as<u64>();
    GHIP(C->timer.start(s));
    GHIP(hipMemsetAsync(C->counters.p, 0, CH_C_N * 8, s)); GHIP(hipMemsetAsync(a.head + na, 0, 1, s));
    GHIP(hipMemsetAsync(C->chain_windows.p, 0, na * 4, s)); GHIP(hipMemsetAsync(C->chain_gap_windows.p, 0, na * 4, s)); GHIP(hipMemsetAsync(C->path_length.p, 0, na * 8, s));
    const unsigned ga = grid_for(na);
    hipLaunchKernelGGL(bridge_kernel, dim3(ga), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    GHIP(excl_scan(C->tmp, (const u8*)a.head, C->cpos.as<u32>(), (size_t)na + 1, s));
    hipLaunchKernelGGL(chain_sum_kernel, dim3(ga), dim3(256), 0, s, a);
    hipLaunchKernelGGL(chain_coord_kernel, dim3(ga), dim3(256), 0, s, a);
    hipLaunchKernelGGL(chain_reads_kernel, dim3(grid_for(nr + 1)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    u64 h[CH_C_N];
    GHIP(C->timer.stop_and_read(h, a.counters, sizeof h, s, &out->ms));
    out->defect = (u32)h[CH_C_DEFECT];
    if (out->defect) return hipSuccess;
    out->n_bridges_inside = h[CH_C_INSIDE]; out->n_bridges_record = h[CH_C_RECORD]; out->n_gap_windows = h[CH_C_GAP]; out->n_chains = h[CH_C_CHAINS];
    out->bridge_record = a.bridge_record; out->bridge_entries = a.bridge_entries; out->chain_offsets = a.chain_offsets; out->chain_aln_offsets = a.chain_aln_offsets;
    out->chain_windows = a.chain_windows; out->chain_gap_windows = a.chain_gap_windows; out->query_begin = a.query_begin; out->query_end = a.query_end;
    out->path_length = a.path_length; out->path_begin = a.path_begin; out->path_end = a.path_end;
    return hipSuccess;
}
