// repeats.hip — the REPEATS step of a simplify schedule: duplicate the unitigs the resident reads resolve, on the GPU (gfx950).  Definition: include/mdbg_hip.h
// (mdbg_graph_simplify, MDBG_SIMPLIFY_REPEATS).  Input, all on the device: the transit result of the current list (transits.hip: the rows in key order, hence
// grouped by unitig, and the verdicts), the arrays the last compaction left in UnitigBuffers (the records' vertices eu / ev, ekeep = the record is a unitig edge
// record, the settled ranking P / D, flag, uid, hoff: node vertex -> unitig and entry), the list, the node columns, the edge records and the two masks.
//
// Coordinates.  A node vertex is v = 2 * row + minus (unitigs.hip); the LIST vertex of the definitions is 2 * (offsets[u] + j) + s (placement_dev.h).  list_vertex
// maps the first to the second through the ranking: v lies on a kept chain (strand 0) or comp(v) does (strand 1), at entry hoff[head] + D.
// Copy (u, i, j), i >= 1, is row n + rowbase[u] + (i - 1) * m(u) + j with index X + C0 + that offset, C0 the copies of the schedule's earlier steps (a NESTED
// step behind a step that copied; else 0); rowbase is a scan over the unitigs, so the order is the definition's (ascending u, then i, then j).  X comes from
// the node table, and a copy's origin is resolved through the earlier steps' origin[], so it always names a table row.
//
// With earlier copies the node columns, records and masks the step reads already live in the x_* blocks: it then grows into FRESH blocks, copies the old contents
// (origin[] included) over, and swaps the blocks in behind its last wait; the old ones go back to the block cache.  Without, it grows the x_* blocks themselves.
//
//   strong_kernel    one thread per transit row: flag = the key is strong and its unitig RESOLVED;  (rocPRIM) rank = exclusive scan of the flags: row d of unitig u
//                    is the strong key number rank[d] - rank[first row of u]
//   size_kernel      one thread per unitig: (m - 1) * m(u) rows if it is resolved, else 0;  (rocPRIM) rowbase = exclusive scan
//   rec_size_kernel  one thread per node-level record: m - 1 new records if it is an interior link of a resolved unitig, else 0;  (rocPRIM) ebase = exclusive scan
//   (read-back)      the two totals and the table's largest index: ONE wait; then the x_* blocks grow and the originals' columns, records and masks are copied
//   copy_kernel      one thread per node vertex of a kept chain of a resolved unitig: its row's columns -> the m - 1 copies, origin[], alive = 1
//   records_kernel   one thread per node-level record.  A unitig edge record: each end at a resolved unitig finds the ONE strong key whose entrance (p) or exit (q)
//                    is the other end (the rows of that unitig: binary search, then a walk over its rows) and names that key's copy; none or two: RX_DEFECT_MATCH
//                    and the end stays.  An interior link of a resolved unitig: its m - 1 copies behind the records, with the same orientations and overlap
//   report_kernel    (end of the schedule) node[] of the list: a copy's index -> its original's
//
// Nothing but sums, scans and searches decides a position: two calls give identical arrays.  The only atomic is the OR into the defect flag.
// Per copied row 52 bytes are written (the seven node columns 47, origin 4, alive 1) and 47 read; per added record 14 (+1 with a record mask); per record of
// the input 12 bytes of temporaries (its count 4, its base 8), per unitig 16, per transit row 5.
#include <cstring>

#include "../../include/mdbg_hip.h"
#include "repeats.h"

namespace {

struct RxArgs {
    // the list and the last compaction
    u64 U, N, E; u32 n, n2x; const u64* offsets;
    const u32* P; const u32* D; const u32* flag; const u32* uid; const u32* hoff; const u32* eu; const u32* ev; const u32* ekeep;
    // the transit result
    u64 T, min_support; const u32* t_unitig; const u32* iu; const u32* ie; const u8* is; const u32* ou; const u32* oe; const u8* os; const u64* count;
    const u32* n_in; const u8* verdict;
    // the step's own
    u8* strong; const u32* rank; u64* rows; const u64* rowbase; u32* ecnt; const u64* ebase; u32* defect;
    u32 X; u64 C, EC;                                       // X: the first index of THIS step's copies; the totals of the two scans: no copy and no added record lies behind them
    u32 X0; u64 C0; const u32* origin0;                     // the earlier steps': their first index (1 + the table's largest), their copies, their origin[]
    UnitigNodes src; EdgeResult esrc;
    u32* x_index; u16* x_abund; u64* x_shift; u64* x_sread; u64* x_sstart; u64* x_send; u8* x_rev; u8* x_alive; u32* x_origin;
    u32* x_n1; u8* x_o1; u32* x_n2; u8* x_o2; u32* x_ov; u8* x_ealive;
};

__device__ inline void rx_defect(const RxArgs& a, u32 what) { atomicOr(a.defect, what); }
__device__ inline bool resolved(const RxArgs& a, u32 u) { return u < a.U && a.verdict[u] == MDBG_TRANSIT_RESOLVED; }
// node vertex v (< n2x, of a surviving node) -> its list vertex, *u <- its unitig; false (with RX_DEFECT_SHAPE): the ranking names something outside the list
__device__ inline bool list_vertex(const RxArgs& a, u32 v, u32* lv, u32* u) {
    u32 w = v, h = a.P[w] & ~TERM, s = 0;
    if (h < a.n2x && !a.flag[h]) { w = v ^ 1u; h = a.P[w] & ~TERM; s = 1; }
    if (h >= a.n2x || !a.flag[h]) { rx_defect(a, RX_DEFECT_SHAPE); return false; }
    const u32 un = a.uid[h];
    const u64 e = (u64)a.hoff[h] + a.D[w];
    if (un >= a.U || e < a.offsets[un] || e >= a.offsets[un + 1]) { rx_defect(a, RX_DEFECT_SHAPE); return false; }
    *u = un; *lv = (u32)(2 * e + s);
    return true;
}
// the row offset (behind n) of copy i >= 1 of entry j of unitig u
__device__ inline u64 copy_of(const RxArgs& a, u32 u, u32 i, u64 j) { return a.rowbase[u] + (u64)(i - 1) * (a.offsets[u + 1] - a.offsets[u]) + j; }

__global__ __launch_bounds__(256) void strong_kernel(RxArgs a) {
    const u64 d = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.T) return;
    a.strong[d] = a.count[d] >= a.min_support && resolved(a, a.t_unitig[d]);
}

__global__ __launch_bounds__(256) void size_kernel(RxArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    const u32 m = a.n_in[u];
    a.rows[u] = resolved(a, (u32)u) && m >= 2 ? (u64)(m - 1) * (a.offsets[u + 1] - a.offsets[u]) : 0;
}

// e is an interior link of a resolved unitig: *u <- the unitig, *j1 / *j2 <- the entries of its two nodes
__device__ inline bool interior_of_resolved(const RxArgs& a, u64 e, u32* u, u64* j1, u64* j2) {
    const u32 x = a.eu[e], y = a.ev[e];
    if (x >= a.n2x || y >= a.n2x || a.ekeep[e]) return false;      // (NONE: an end or the record was removed)
    u32 lx, ly, ux, uy;
    if (!list_vertex(a, x, &lx, &ux) || !list_vertex(a, y, &ly, &uy)) return false;
    if (ux != uy) { rx_defect(a, RX_DEFECT_SHAPE); return false; }
    if (!resolved(a, ux)) return false;
    *u = ux; *j1 = (lx >> 1) - a.offsets[ux]; *j2 = (ly >> 1) - a.offsets[ux];
    return true;
}

__global__ __launch_bounds__(256) void rec_size_kernel(RxArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    u32 u; u64 j1, j2;
    a.ecnt[e] = interior_of_resolved(a, e, &u, &j1, &j2) && a.n_in[u] >= 2 ? a.n_in[u] - 1 : 0u;
}

__global__ __launch_bounds__(256) void copy_kernel(RxArgs a) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n2x) return;
    const u32 h = a.P[v] & ~TERM;
    if (h >= a.n2x || !a.flag[h]) return;                   // the kept chains hold every surviving node once
    u32 lv, u;
    if (!list_vertex(a, v, &lv, &u) || !resolved(a, u)) return;
    const u32 r = v >> 1, m = a.n_in[u];
    const u64 j = (lv >> 1) - a.offsets[u];
    const u32 index = a.src.index[r]; const u16 abund = a.src.abund[r]; const u64 s0 = a.src.shift_full[2 * (u64)r], s1 = a.src.shift_full[2 * (u64)r + 1];
    const u64 sread = a.src.src_read[r], sstart = a.src.src_start[r], send = a.src.src_end[r]; const u8 rev = a.src.reversed[r];
    for (u32 i = 1; i < m; ++i) {
        const u64 c = copy_of(a, u, i, j), d = (u64)a.n + c;
        if (c >= a.C) { rx_defect(a, RX_DEFECT_SHAPE); return; }      // cannot happen (the host has sized the blocks by the scan's total); never write outside
        a.x_index[d] = a.X + (u32)c; a.x_abund[d] = abund; a.x_shift[2 * d] = s0; a.x_shift[2 * d + 1] = s1;
        a.x_sread[d] = sread; a.x_sstart[d] = sstart; a.x_send[d] = send; a.x_rev[d] = rev; a.x_alive[d] = 1;
            a.x_origin[c] = index >= a.X0 && (u64)(index - a.X0) < a.C0 ? a.origin0[index - a.X0] : index;      // (x_origin: this step's part of the array)
    }
}

// the strong key of resolved unitig u whose exit (by_exit) or entrance is the list vertex `other`: its number i, or NONE with RX_DEFECT_MATCH
__device__ inline u32 key_with(const RxArgs& a, u32 u, bool by_exit, u32 other) {
    u64 lo = 0, hi = a.T;                                   // the first row of u (the rows are in key order: ascending unitig)
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.t_unitig[mid] < u) lo = mid + 1; else hi = mid; }
    const u64 d0 = lo;
    u32 found = 0, i = NONE;
    for (u64 d = d0; d < a.T && a.t_unitig[d] == u; ++d) {
        if (!a.strong[d]) continue;
        const u32 vu = by_exit ? a.ou[d] : a.iu[d], ve = by_exit ? a.oe[d] : a.ie[d], vs = by_exit ? a.os[d] : a.is[d];
        if (vu >= a.U) { rx_defect(a, RX_DEFECT_SHAPE); return NONE; }
        if ((u32)(2 * (a.offsets[vu] + ve) + vs) == other) { ++found; i = a.rank[d] - a.rank[d0]; }
    }
    if (found != 1 || i >= a.n_in[u]) { rx_defect(a, RX_DEFECT_MATCH); return NONE; }
    return i;
}

__global__ __launch_bounds__(256) void records_kernel(RxArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const u32 x = a.eu[e], y = a.ev[e];
    if (x >= a.n2x || y >= a.n2x) return;                   // no record of the current graph: it stays as it was copied
    if (!a.ekeep[e]) {                                      // an interior link: its copies
        const u32 cnt = a.ecnt[e];
        if (!cnt) return;
        u32 u; u64 j1, j2;
        if (!interior_of_resolved(a, e, &u, &j1, &j2) || cnt != a.n_in[u] - 1) return;
        const u8 o1 = a.esrc.o1[e], o2 = a.esrc.o2[e]; const u32 ov = a.esrc.overlap[e];
        for (u32 i = 1; i <= cnt; ++i) {
            const u64 d = a.E + a.ebase[e] + (i - 1);
            if (d >= a.E + a.EC) { rx_defect(a, RX_DEFECT_SHAPE); return; }
            a.x_n1[d] = a.X + (u32)copy_of(a, u, i, j1); a.x_o1[d] = o1; a.x_n2[d] = a.X + (u32)copy_of(a, u, i, j2); a.x_o2[d] = o2; a.x_ov[d] = ov;
            if (a.x_ealive) a.x_ealive[d] = 1;
        }
        return;
    }
    u32 lx, ly, ux, uy;
    if (!list_vertex(a, x, &lx, &ux) || !list_vertex(a, y, &ly, &uy)) return;
    if (resolved(a, ux)) {                                  // the source end
        const u32 first = (u32)(a.offsets[ux] << 1), last = (u32)((a.offsets[ux + 1] - 1) << 1);
        u32 i = 0;
        if (lx == last) i = key_with(a, ux, true, ly);                      // x == (u, m - 1, 0): the key with q == y
        else if (lx == (first | 1u)) i = key_with(a, ux, false, ly ^ 1u);   // x == (u, 0, 1): the key with p == comp(y)
        else rx_defect(a, RX_DEFECT_SHAPE);                                 // (a unitig edge record leaves a unitig at one of its two ends)
        if (i != NONE && i > 0) a.x_n1[e] = a.X + (u32)copy_of(a, ux, i, (lx >> 1) - a.offsets[ux]);
    }
    if (resolved(a, uy)) {                                  // the target end
        const u32 first = (u32)(a.offsets[uy] << 1), last = (u32)((a.offsets[uy + 1] - 1) << 1);
        u32 i = 0;
        if (ly == first) i = key_with(a, uy, false, lx);                    // y == (u, 0, 0): the key with p == x
        else if (ly == (last | 1u)) i = key_with(a, uy, true, lx ^ 1u);     // y == (u, m - 1, 1): the key with q == comp(x)
        else rx_defect(a, RX_DEFECT_SHAPE);
        if (i != NONE && i > 0) a.x_n2[e] = a.X + (u32)copy_of(a, uy, i, (ly >> 1) - a.offsets[uy]);
    }
}

__global__ __launch_bounds__(256) void report_kernel(u64 n_entries, u32* __restrict__ node, u32 X, u64 copies, const u32* __restrict__ origin) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const u32 idx = node[i];
    if (idx >= X && (u64)(idx - X) < copies) node[i] = origin[idx - X];
}

}  // namespace

namespace {
void swap_blocks(Buf& a, Buf& b) { void* p = a.p; a.p = b.p; b.p = p; const size_t c = a.cap; a.cap = b.cap; b.cap = c; }
}  // namespace

hipError_t repeats_run(UnitigBuffers* B, const TransitResult& tr, uint64_t min_support, const UnitigResult& ul, const UnitigNodes& nd, const EdgeResult& ed, const uint8_t* alive,
                       const uint8_t* edge_alive, const uint32_t* table_last_index, const RepeatsResult* earlier, hipStream_t s, RepeatsResult* out) {
    const u64 C0 = earlier ? earlier->total_copies : 0;
    const u32* origin0 = C0 ? earlier->origin : nullptr;
    memset(out, 0, sizeof *out);
    const u64 n = nd.n, E = ed.n, U = ul.n_unitigs, T = tr.n_transits;
    if (n == 0 || n >= (1ull << 30) || E == 0 || U == 0 || T == 0 || tr.n_unitigs != U || !alive) return hipErrorInvalidValue;
    // every buffer of the first half, then the launches (growing a block may wait for the device: graph_common.h)
    GHIP(B->x_strong.ensure(T)); GHIP(B->x_rank.ensure(T * 4)); GHIP(B->x_rows.ensure(U * 8)); GHIP(B->x_rowbase.ensure(U * 8));
    GHIP(B->x_ecnt.ensure(E * 4)); GHIP(B->x_ebase.ensure(E * 8)); GHIP(B->x_ctr.ensure(4));
    RxArgs a; memset(&a, 0, sizeof a);
    a.U = U; a.N = ul.n_entries; a.E = E; a.n = (u32)n; a.n2x = (u32)(2 * n); a.offsets = ul.offsets;
    a.P = B->Pfin; a.D = B->Dfin; a.flag = B->flag.as<u32>(); a.uid = B->uid.as<u32>(); a.hoff = B->hoff.as<u32>(); a.eu = B->eu.as<u32>(); a.ev = B->ev.as<u32>(); a.ekeep = B->ekeep.as<u32>();
    a.T = T; a.min_support = min_support; a.t_unitig = tr.unitig; a.iu = tr.in_unitig; a.ie = tr.in_entry; a.is = tr.in_strand; a.ou = tr.out_unitig; a.oe = tr.out_entry; a.os = tr.out_strand;
    a.count = tr.count; a.n_in = tr.n_in; a.verdict = tr.verdict;
    a.strong = B->x_strong.as<u8>(); a.rank = B->x_rank.as<u32>(); a.rows = B->x_rows.as<u64>(); a.rowbase = B->x_rowbase.as<u64>(); a.ecnt = B->x_ecnt.as<u32>(); a.ebase = B->x_ebase.as<u64>();
    a.defect = B->x_ctr.as<u32>(); a.src = nd; a.esrc = ed;
    GHIP(hipMemsetAsync(B->x_ctr.p, 0, 4, s));
    hipLaunchKernelGGL(strong_kernel, dim3(grid_for(T)), dim3(256), 0, s, a);
    GHIP(excl_scan(B->tmp, (const u8*)a.strong, B->x_rank.as<u32>(), (size_t)T, s));
    hipLaunchKernelGGL(size_kernel, dim3(grid_for(U)), dim3(256), 0, s, a);
    GHIP(excl_scan(B->tmp, (const u64*)a.rows, B->x_rowbase.as<u64>(), (size_t)U, s));
    hipLaunchKernelGGL(rec_size_kernel, dim3(grid_for(E)), dim3(256), 0, s, a);
    GHIP(excl_scan(B->tmp, (const u32*)a.ecnt, B->x_ebase.as<u64>(), (size_t)E, s));
    GHIP(hipGetLastError());
    ScanLast<u64, u64> rows; ScanLast<u32, u64> recs; u32 largest = 0;
    GHIP(scan_total((const u64*)a.rows, a.rowbase, (size_t)U, s, &rows));
    GHIP(scan_total((const u32*)a.ecnt, a.ebase, (size_t)E, s, &recs));
    GHIP(hipMemcpyAsync(&largest, table_last_index, 4, hipMemcpyDeviceToHost, s));      // (the table is sorted by index)
    GHIP(hipStreamSynchronize(s));
    const u64 C = rows.total(), EC = recs.total(), n2 = n + C, E2 = E + EC;
    if (n2 >= (1ull << 30) || E2 >= 0xFFFFFFF0ull || (u64)largest + 1 + C0 + C >= 0xFFFFFFF0ull) { out->too_large = true; return hipSuccess; }
    const u32 X0 = largest + 1;
    // where the extended arrays go: the x_* blocks, or fresh ones when the step reads the x_* blocks (they are swapped in below)
    enum { I_INDEX, I_ABUND, I_SHIFT, I_SREAD, I_SSTART, I_SEND, I_REV, I_ALIVE, I_ORIGIN, I_N1, I_N2, I_OV, I_O1, I_O2, I_EALIVE, I_N };
    Buf fresh[I_N];
    Buf* const mine[I_N] = {&B->x_index, &B->x_abund, &B->x_shift, &B->x_sread, &B->x_sstart, &B->x_send, &B->x_rev, &B->x_alive, &B->x_origin, &B->x_n1, &B->x_n2, &B->x_ov, &B->x_o1, &B->x_o2, &B->x_ealive};
    Buf* to[I_N];
    for (int q = 0; q < I_N; ++q) to[q] = C0 ? &fresh[q] : mine[q];
    GHIP(to[I_INDEX]->ensure(n2 * 4)); GHIP(to[I_ABUND]->ensure(n2 * 2)); GHIP(to[I_SHIFT]->ensure(n2 * 16)); GHIP(to[I_SREAD]->ensure(n2 * 8)); GHIP(to[I_SSTART]->ensure(n2 * 8));
    GHIP(to[I_SEND]->ensure(n2 * 8)); GHIP(to[I_REV]->ensure(n2)); GHIP(to[I_ALIVE]->ensure(n2)); GHIP(to[I_ORIGIN]->ensure((C0 + C) * 4 + 4));
    GHIP(to[I_N1]->ensure(E2 * 4)); GHIP(to[I_N2]->ensure(E2 * 4)); GHIP(to[I_OV]->ensure(E2 * 4)); GHIP(to[I_O1]->ensure(E2)); GHIP(to[I_O2]->ensure(E2));
    if (edge_alive) GHIP(to[I_EALIVE]->ensure(E2));
    a.X = X0 + (u32)C0; a.C = C; a.EC = EC; a.X0 = X0; a.C0 = C0; a.origin0 = origin0;
    a.x_index = to[I_INDEX]->as<u32>(); a.x_abund = to[I_ABUND]->as<u16>(); a.x_shift = to[I_SHIFT]->as<u64>(); a.x_sread = to[I_SREAD]->as<u64>(); a.x_sstart = to[I_SSTART]->as<u64>();
    a.x_send = to[I_SEND]->as<u64>(); a.x_rev = to[I_REV]->as<u8>(); a.x_alive = to[I_ALIVE]->as<u8>(); a.x_origin = to[I_ORIGIN]->as<u32>() + C0;
    a.x_n1 = to[I_N1]->as<u32>(); a.x_o1 = to[I_O1]->as<u8>(); a.x_n2 = to[I_N2]->as<u32>(); a.x_o2 = to[I_O2]->as<u8>(); a.x_ov = to[I_OV]->as<u32>(); a.x_ealive = edge_alive ? to[I_EALIVE]->as<u8>() : nullptr;
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    if (C0) GHIP(hipMemcpyAsync(to[I_ORIGIN]->p, origin0, C0 * 4, dd, s));
    GHIP(hipMemcpyAsync(a.x_index, nd.index, n * 4, dd, s)); GHIP(hipMemcpyAsync(a.x_abund, nd.abund, n * 2, dd, s)); GHIP(hipMemcpyAsync(a.x_shift, nd.shift_full, n * 16, dd, s));
    GHIP(hipMemcpyAsync(a.x_sread, nd.src_read, n * 8, dd, s)); GHIP(hipMemcpyAsync(a.x_sstart, nd.src_start, n * 8, dd, s)); GHIP(hipMemcpyAsync(a.x_send, nd.src_end, n * 8, dd, s));
    GHIP(hipMemcpyAsync(a.x_rev, nd.reversed, n, dd, s)); GHIP(hipMemcpyAsync(a.x_alive, alive, n, dd, s));
    GHIP(hipMemcpyAsync(a.x_n1, ed.n1, E * 4, dd, s)); GHIP(hipMemcpyAsync(a.x_n2, ed.n2, E * 4, dd, s)); GHIP(hipMemcpyAsync(a.x_ov, ed.overlap, E * 4, dd, s));
    GHIP(hipMemcpyAsync(a.x_o1, ed.o1, E, dd, s)); GHIP(hipMemcpyAsync(a.x_o2, ed.o2, E, dd, s));
    if (edge_alive) GHIP(hipMemcpyAsync(a.x_ealive, edge_alive, E, dd, s));
    hipLaunchKernelGGL(copy_kernel, dim3(grid_for(a.n2x)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(records_kernel, dim3(grid_for(E)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    GHIP(hipMemcpyAsync(&out->defect, a.defect, 4, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));
    if (C0) for (int q = 0; q < I_N; ++q) swap_blocks(*mine[q], fresh[q]);      // (the device is idle: the old blocks are read by nobody)
    out->nd.index = a.x_index; out->nd.abund = a.x_abund; out->nd.shift_full = a.x_shift; out->nd.src_read = a.x_sread; out->nd.src_start = a.x_sstart; out->nd.src_end = a.x_send;
    out->nd.reversed = a.x_rev; out->nd.n = n2;
    out->ed = ed; out->ed.n = E2; out->ed.n1 = a.x_n1; out->ed.o1 = a.x_o1; out->ed.n2 = a.x_n2; out->ed.o2 = a.x_o2; out->ed.overlap = a.x_ov;
    out->alive = a.x_alive; out->edge_alive = a.x_ealive; out->copies = C; out->total_copies = C0 + C; out->records_added = EC; out->first_copy_index = X0; out->origin = a.x_origin - C0;
    return hipSuccess;
}

hipError_t repeats_report_originals(UnitigBuffers* B, const UnitigResult& ul, const RepeatsResult& r, hipStream_t s) {
    if (ul.n_entries == 0 || r.total_copies == 0) return hipSuccess;
    hipLaunchKernelGGL(report_kernel, dim3(grid_for(ul.n_entries)), dim3(256), 0, s, ul.n_entries, B->node.as<u32>(), r.first_copy_index, r.total_copies, r.origin);
    return hipGetLastError();
}
