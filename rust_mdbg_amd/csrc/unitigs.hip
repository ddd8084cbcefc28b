// unitigs.hip — unitig compaction of the k-min-mer graph and the base-space copy plan, on the GPU (gfx950).
//
// Replaces the two tools every documented rust-mdbg run pipes its .gfa through: `gfatools asm -u` (compaction of non-branching paths) and
// the part of src/to_basespace.rs that decides which piece of which node sequence goes where in a unitig (:132-153, 203-262).  Tip and
// bubble removal is simplify.hip (a translation unit of its own: it decides on this stage's arrays, which unitigs_priv.h shows it, and compacts again under a node mask).  Input: the node table of the last finalize and the edge list of the last edge call, both resident on the device.
//
// Vertex v = 2 * row + (orientation == '-'), comp(v) = v ^ 1; rows are positions in the index-sorted node table, so vertex order is
// (index, orientation) order.  The arc set is the set of DISTINCT (n1,o1)->(n2,o2) of the edge records plus their mirrors
// comp(v)->comp(u), hence closed under mirroring: the in-degree of v is the out-degree of comp(v), and ONE sort of the 2E arcs by
// (source, target) gives every degree the link test needs — no second sort, no degree atomics.
//
//   arc_kernel       edge record -> its two vertices (binary search of index -> row) and its two arcs as u64 keys; rocPRIM sorts them.  Under simplify.hip's
//                    masks a record with a removed end, or a removed record, gets no vertices and two arcs at source 2n, behind every vertex
//   succ_kernel      first arc of every source group: the unique successor if the group holds one distinct target
//   link_kernel      u->v is a link iff u has one distinct out-arc, v one distinct in-arc, node(u) != node(v); next / prev per vertex and the
//                    start state of the ranking
//   jump_kernel      pointer jumping towards the chain head: pointer, distance and the smallest vertex of the span, ping-pong buffers.
//                    A pointer carries TERM once it names the head and the distance is final.  After r rounds every vertex within
//                    2^r - 1 links of a head is final, so ceil(log2(2n)) + 1 rounds settle every path; a round that settles nothing
//                    leaves only cycles, whose span minimum is complete once 2^rounds covers the vertices left
//   cut_kernel       a cycle's smallest vertex becomes its head (the pointer into it is cut), then the same jumping ranks the cycles
//   head_kernel      per head: tail, length, and whether this chain or its mirror is the unitig (canonical orientation)
//   emit_kernel      walk entry of every vertex of a kept chain at offset[unitig] + rank, with its copy-plan piece
//   finish_kernel    dst_offset / LN / abundance sum from two global scans, cut at the unitig boundaries (= a segmented scan)
//   uedge_*          edge records that are not interior links -> unitig edges, in source order, overlaps clamped (to_basespace.rs:312-320)
#include <cstring>

#include "unitigs_priv.h"

namespace {

enum { C_ERR = 62, C_NONTERM = 63, N_CTR = 64 };      // counters: [round] = vertices not final after that round

// row of the node with DbgEntry.index == idx (the table is sorted by index); NONE if absent
__device__ inline u32 row_of(const u32* __restrict__ index, u32 n, u32 idx) {
    u32 lo = 0, hi = n;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (index[mid] < idx) lo = mid + 1; else hi = mid; }
    return (lo < n && index[lo] == idx) ? lo : NONE;
}

__global__ __launch_bounds__(256) void arc_kernel(u64 n_edges, const u32* __restrict__ n1, const u8* __restrict__ o1, const u32* __restrict__ n2, const u8* __restrict__ o2,
                                                  const u32* __restrict__ index, u32 n, const u8* __restrict__ alive, const u8* __restrict__ edge_alive, u32* __restrict__ eu, u32* __restrict__ ev, u64* __restrict__ keys,
                                                  u32* __restrict__ ctr) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const u32 ra = row_of(index, n, n1[e]), rb = row_of(index, n, n2[e]);
    // an end was removed, or the record itself (simplify.hip): no vertices, and both arcs sort behind every vertex (source 2n)
    if (ra != NONE && rb != NONE && ((alive && !(alive[ra] && alive[rb])) || (edge_alive && !edge_alive[e]))) {
        eu[e] = NONE; ev[e] = NONE; keys[2 * e] = (u64)(2 * n) << 32; keys[2 * e + 1] = (u64)(2 * n) << 32; return;
    }
    if (ra == NONE || rb == NONE) { ctr[C_ERR] = 1; eu[e] = 0; ev[e] = 0; keys[2 * e] = 0; keys[2 * e + 1] = 0; return; }      // an edge of another table: reported by the host
    const u32 u = 2 * ra + (o1[e] == '-' ? 1u : 0u), v = 2 * rb + (o2[e] == '-' ? 1u : 0u);
    eu[e] = u; ev[e] = v;
    keys[2 * e] = ((u64)u << 32) | v;
    keys[2 * e + 1] = ((u64)(v ^ 1) << 32) | (u ^ 1);      // the mirror arc
}

// sorted arcs: the first arc of a source group writes the group's only target, if it has only one
__global__ __launch_bounds__(256) void succ_kernel(u64 n_arcs, u32 n2x, const u64* __restrict__ sk, u32* __restrict__ succ) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_arcs) return;
    const u64 key = sk[i];
    const u32 src = (u32)(key >> 32);
    if (src >= n2x) return;                               // arcs of removed nodes
    if (i > 0 && (u32)(sk[i - 1] >> 32) == src) return;
    u64 lo = i + 1, hi = n_arcs;                          // first arc > key (duplicates of key are skipped)
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (sk[mid] <= key) lo = mid + 1; else hi = mid; }
    if (lo < n_arcs && (u32)(sk[lo] >> 32) == src) return;       // a second distinct target
    succ[src] = (u32)key;
}

__device__ inline u32 link_from(const u32* __restrict__ succ, u32 u) {      // v if u->v is a link, else NONE
    const u32 v = succ[u];
    if (v == NONE || (v >> 1) == (u >> 1)) return NONE;
    return succ[v ^ 1] == NONE ? NONE : v;                // in-degree of v = out-degree of comp(v); its only arc is then the mirror of u->v
}

__global__ __launch_bounds__(256) void link_kernel(u32 n2x, const u32* __restrict__ succ, u32* __restrict__ nxt, u32* __restrict__ prv, u32* __restrict__ P, u32* __restrict__ D,
                                                   u32* __restrict__ M, u32* __restrict__ ctr) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    bool nonterm = false;
    if (v < n2x) {
        nxt[v] = link_from(succ, v);
        const u32 m = link_from(succ, v ^ 1);             // comp(v) -> m is a link iff comp(m) -> v is
        const u32 pv = m == NONE ? NONE : (m ^ 1);
        prv[v] = pv;
        nonterm = pv != NONE;
        P[v] = nonterm ? pv : (v | TERM); D[v] = nonterm ? 1u : 0u; M[v] = nonterm && pv < v ? pv : v;
    }
    count_to(ctr + C_NONTERM, nonterm);
}

__global__ __launch_bounds__(256) void jump_kernel(u32 n2x, const u32* __restrict__ Pi, const u32* __restrict__ Di, const u32* __restrict__ Mi, u32* __restrict__ Po,
                                                   u32* __restrict__ Do, u32* __restrict__ Mo, u32* __restrict__ ctr_round) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    bool open = false;
    if (v < n2x) {
        u32 p = Pi[v], d = Di[v], m = Mi[v];
        if (!(p & TERM)) {
            const u32 mp = Mi[p];
            d += Di[p]; m = mp < m ? mp : m; p = Pi[p];   // p's pointer: final (TERM) if p was, else p's own jump
            open = !(p & TERM);
        }
        Po[v] = p; Do[v] = d; Mo[v] = m;
    }
    count_to(ctr_round, open);
}

// what is still open after the paths settled lies on cycles: the smallest vertex of each becomes its head
__global__ __launch_bounds__(256) void cut_kernel(u32 n2x, const u32* __restrict__ prv, u32* __restrict__ P, u32* __restrict__ D, const u32* __restrict__ M, u8* __restrict__ cyc) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n2x || (P[v] & TERM)) return;
    cyc[v] = 1;
    const bool head = M[v] == v;
    P[v] = head ? (v | TERM) : prv[v]; D[v] = head ? 0u : 1u;
}

// heads: is this chain the unitig or is its mirror?  linear: the first node has the smaller index (one node: '+'); circular: the smallest vertex is a '+'
__global__ __launch_bounds__(256) void head_kernel(u32 n2x, const u32* __restrict__ P, const u32* __restrict__ D, const u32* __restrict__ prv, const u8* __restrict__ cyc,
                                                   const u8* __restrict__ alive, u32* __restrict__ flag, u32* __restrict__ hlen) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n2x) return;
    u32 keep = 0, len = 0;
    if ((P[v] & ~TERM) == v && (!alive || alive[v >> 1])) {      // (a removed node has no arcs: its vertices are heads of nothing)
        u32 t;                                            // the chain's last vertex
        if (cyc && cyc[v]) { t = prv[v]; keep = (v & 1) ? 0u : 1u; }
        else { t = (P[v ^ 1] & ~TERM) ^ 1; keep = ((v >> 1) < (t >> 1) || (v == t && !(v & 1))) ? 1u : 0u; }      // comp(v) ends the mirror chain, whose head is comp(t)
        if (keep) len = D[t] + 1;
    }
    flag[v] = keep; hlen[v] = len;
}

struct EmitArgs {
    UnitigNodes nd; u32 n2x; u64 n_unitigs, n_entries;
    const u32* P; const u32* D; const u32* flag; const u32* uid; const u32* hoff; const u8* cyc;
    u64* offsets; u8* circular;
    u32* node; u8* ori; u64* src_read; u64* src_begin; u32* len; u8* rc; u32* ent_u; u64* pl64; u64* ab64;
};

// one walk entry per vertex of a kept chain.  Copy plan in READ coordinates by the rule of to_basespace.rs:203-262 — with seq = the node's .sequences
// sequence = read[a, b), reverse-complemented when `reversed` (main.rs:700-701), and (s0, s1) = shift_full:
//   first entry  '+' all of seq, '-' revcomp(seq);   later entries  '+' the last s1 bases of seq, '-' revcomp of the first s0 bases.
// rc counts the reverse complements between the read and the unitig (0, 1, or 2 = forward again, but through utils::revcomp's byte map twice).
__global__ __launch_bounds__(256) void emit_kernel(EmitArgs a) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) { a.offsets[a.n_unitigs] = a.n_entries; a.pl64[a.n_entries] = 0; a.ab64[a.n_entries] = 0; }
    if (v >= a.n2x) return;
    const u32 h = a.P[v] & ~TERM;
    if (!a.flag[h]) return;
    const u32 u = a.uid[h], rank = a.D[v];
    if (rank == 0) { a.offsets[u] = a.hoff[h]; a.circular[u] = a.cyc ? a.cyc[h] : (u8)0; }
    const u64 pos = (u64)a.hoff[h] + rank;
    if (pos >= a.n_entries) return;                       // cannot happen (the host has checked the totals); never write outside
    const u32 r = v >> 1; const bool minus = (v & 1) != 0, rev = a.nd.reversed[r] != 0;
    const u64 s = a.nd.src_start[r], e = a.nd.src_end[r], L = e > s ? e - s : 0;
    u64 begin = s, n = L;
    if (rank) {
        const u64 sh = a.nd.shift_full[2 * r + (minus ? 0 : 1)];
        n = sh < L ? sh : L;
        begin = (minus == rev) ? e - n : s;               // '+' of a forward node / '-' of a reversed one take the read's right end
    }
    a.node[pos] = a.nd.index[r]; a.ori[pos] = minus ? '-' : '+';
    a.src_read[pos] = a.nd.src_read[r]; a.src_begin[pos] = begin; a.len[pos] = (u32)n; a.rc[pos] = (u8)((rev ? 1 : 0) + (minus ? 1 : 0));
    a.ent_u[pos] = u; a.pl64[pos] = n; a.ab64[pos] = a.nd.abund[r];
}

__global__ __launch_bounds__(256) void finish_kernel(u64 n_entries, u64 n_unitigs, const u64* __restrict__ offsets, const u32* __restrict__ ent_u, const u64* __restrict__ gs,
                                                     const u64* __restrict__ ga, u64* __restrict__ dst, u64* __restrict__ length, u64* __restrict__ kc) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_entries) dst[i] = gs[i] - gs[offsets[ent_u[i]]];
    if (i < n_unitigs) { const u64 a = offsets[i], b = offsets[i + 1]; length[i] = gs[b] - gs[a]; kc[i] = ga[b] - ga[a]; }
}

struct UedgeArgs {
    u64 n_edges; const u32* eu; const u32* ev; const u32* ov_in; const u32* nxt; const u32* P; const u32* flag; const u32* uid; const u64* length;
    u32* keep; const u32* pos; u32* n1; u8* o1; u32* n2; u8* o2; u32* ov;
};
__device__ inline u32 unitig_of(const UedgeArgs& a, u32 v, bool* minus) {      // v lies on a kept chain ('+') or its complement does ('-')
    u32 h = a.P[v] & ~TERM;
    *minus = !a.flag[h];
    if (*minus) h = a.P[v ^ 1] & ~TERM;
    return a.uid[h];
}
template <bool WRITE>
__global__ __launch_bounds__(256) void uedge_kernel(UedgeArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_edges) return;
    const u32 u = a.eu[e], v = a.ev[e];
    if (u == NONE) { if (!WRITE) a.keep[e] = 0; return; }      // a record of a removed node, or a removed record
    // interior link: a link that is not the closing link of a circular unitig (its target is the kept head) nor that link's mirror (its source is the head's complement);
    // a path has no link into its head, and the mirror cycle's own cut lies elsewhere, so only kept heads count
    if (!WRITE) { a.keep[e] = (a.nxt[u] == v && !a.flag[v] && !a.flag[u ^ 1]) ? 0u : 1u; return; }
    if (!a.keep[e]) return;
    bool m1, m2;
    const u32 a1 = unitig_of(a, u, &m1), a2 = unitig_of(a, v, &m2);
    const u64 l1 = a.length[a1], l2 = a.length[a2];
    u64 ov = a.ov_in[e];
    if (ov > l1 || ov > l2) { const u64 x = l1 ? l1 - 1 : 0, y = l2 ? l2 - 1 : 0; ov = x < y ? x : y; }      // to_basespace.rs:315-319
    const u32 d = a.pos[e];
    a.n1[d] = a1; a.o1[d] = m1 ? '-' : '+'; a.n2[d] = a2; a.o2[d] = m2 ? '-' : '+'; a.ov[d] = (u32)ov;
}

}  // namespace

UnitigBuffers* unitig_buffers_create() { return new UnitigBuffers(); }
void unitig_buffers_destroy(UnitigBuffers* b) { delete b; }

hipError_t build_unitigs_masked(UnitigBuffers* B, const UnitigNodes& nd, const EdgeResult& ed, const u8* alive, u64 n_alive, const u8* edge_alive, hipStream_t s, UnitigResult* out, int* broken) {
    memset(out, 0, sizeof *out);
    *broken = 0;
    const u64 n = nd.n, E = ed.n;
    if (n == 0 || (alive && n_alive == 0)) return hipSuccess;
    if (n >= (1ull << 30) || E >= (1ull << 31)) return defect(broken);
    const u32 n2x = (u32)(2 * n);
    const unsigned gv = grid_for(n2x);
    u32 ctr[N_CTR];
    GHIP(B->ctr.ensure(N_CTR * 4));
    GHIP(hipMemsetAsync(B->ctr.p, 0, N_CTR * 4, s));
    u32* d_ctr = B->ctr.as<u32>();
    // ---- arcs of the edge records and their mirrors, sorted by (source, target); unique successor per vertex
    GHIP(B->succ.ensure((size_t)n2x * 4));
    GHIP(hipMemsetAsync(B->succ.p, 0xFF, (size_t)n2x * 4, s));
    GHIP(B->eu.ensure(E * 4 + 4)); GHIP(B->ev.ensure(E * 4 + 4));
    if (E) {
        GHIP(B->keys.ensure(2 * E * 8)); GHIP(B->skeys.ensure(2 * E * 8));
        hipLaunchKernelGGL(arc_kernel, dim3(grid_for(E)), dim3(256), 0, s, E, ed.n1, ed.o1, ed.n2, ed.o2, nd.index, (u32)n, alive, edge_alive, B->eu.as<u32>(), B->ev.as<u32>(), B->keys.as<u64>(), d_ctr);
        unsigned end_bit = 33; while (end_bit < 64 && (1ull << (end_bit - 32)) < (u64)n2x + (alive || edge_alive ? 1 : 0)) ++end_bit;      // (either mask: the source 2n occurs)
        GHIP(sort_keys(B->tmp, B->keys.as<u64>(), B->skeys.as<u64>(), (size_t)(2 * E), 0, end_bit, s));
        hipLaunchKernelGGL(succ_kernel, dim3(grid_for(2 * E)), dim3(256), 0, s, 2 * E, n2x, B->skeys.as<u64>(), B->succ.as<u32>());
    }
    // ---- links, start state of the ranking
    GHIP(B->nxt.ensure((size_t)n2x * 4)); GHIP(B->prv.ensure((size_t)n2x * 4));
    for (int i = 0; i < 2; ++i) { GHIP(B->P[i].ensure((size_t)n2x * 4)); GHIP(B->D[i].ensure((size_t)n2x * 4)); GHIP(B->M[i].ensure((size_t)n2x * 4)); }
    hipLaunchKernelGGL(link_kernel, dim3(gv), dim3(256), 0, s, n2x, B->succ.as<u32>(), B->nxt.as<u32>(), B->prv.as<u32>(), B->P[0].as<u32>(), B->D[0].as<u32>(), B->M[0].as<u32>(), d_ctr);
    GHIP(hipMemcpyAsync(ctr, d_ctr, N_CTR * 4, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));
    if (ctr[C_ERR]) return defect(broken);
    // ---- pointer jumping: paths first; what stays open lies on cycles
    u32 bound = 1; while ((1ull << (bound - 1)) < n2x) ++bound;      // ceil(log2(2n)) + 1
    u32 open = ctr[C_NONTERM], rounds = 0; int cur = 0;
    bool cycles = false;
    auto jump = [&]() -> hipError_t {
        hipLaunchKernelGGL(jump_kernel, dim3(gv), dim3(256), 0, s, n2x, B->P[cur].as<u32>(), B->D[cur].as<u32>(), B->M[cur].as<u32>(), B->P[cur ^ 1].as<u32>(), B->D[cur ^ 1].as<u32>(),
                           B->M[cur ^ 1].as<u32>(), d_ctr + (rounds % C_ERR));
        cur ^= 1;
        hipError_t e = hipMemcpyAsync(&ctr[0], d_ctr + (rounds % C_ERR), 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        ++rounds;
        return e;
    };
    while (open) {
        if (rounds >= bound) return defect(broken);
        GHIP(jump());
        if (ctr[0] == open) { cycles = true; break; }      // a round that settles nothing: no path vertex is left
        open = ctr[0];
    }
    if (cycles) {
        while ((1ull << rounds) < open) { if (rounds >= bound) return defect(broken); GHIP(jump()); if (ctr[0] != open) return defect(broken); }      // span minimum over whole cycles
        GHIP(B->cyc.ensure(n2x));
        GHIP(hipMemsetAsync(B->cyc.p, 0, n2x, s));
        hipLaunchKernelGGL(cut_kernel, dim3(gv), dim3(256), 0, s, n2x, B->prv.as<u32>(), B->P[cur].as<u32>(), B->D[cur].as<u32>(), B->M[cur].as<u32>(), B->cyc.as<u8>());
        GHIP(hipMemsetAsync(d_ctr, 0, C_ERR * 4, s));
        const u32 bound2 = rounds + bound;
        while (open) {
            if (rounds >= bound2) return defect(broken);
            GHIP(jump());
            if (ctr[0] >= open) return defect(broken);                  // every cycle has a head now: each round must settle something
            open = ctr[0];
        }
    }
    const u32* P = B->P[cur].as<u32>(); const u32* D = B->D[cur].as<u32>();
    const u8* cyc = cycles ? B->cyc.as<u8>() : nullptr;
    // ---- kept heads -> unitig numbers (vertex order = order of the first node's index) and entry offsets
    GHIP(B->flag.ensure((size_t)n2x * 4)); GHIP(B->hlen.ensure((size_t)n2x * 4)); GHIP(B->uid.ensure((size_t)n2x * 4)); GHIP(B->hoff.ensure((size_t)n2x * 4));
    hipLaunchKernelGGL(head_kernel, dim3(gv), dim3(256), 0, s, n2x, P, D, B->prv.as<u32>(), cyc, alive, B->flag.as<u32>(), B->hlen.as<u32>());
    GHIP(excl_scan(B->tmp, B->flag.as<u32>(), B->uid.as<u32>(), n2x, s));
    GHIP(excl_scan(B->tmp, B->hlen.as<u32>(), B->hoff.as<u32>(), n2x, s));
    ScanLast<u32, u32> heads, entries, uedges;
    GHIP(scan_total(B->flag.as<u32>(), B->uid.as<u32>(), n2x, s, &heads));
    GHIP(scan_total(B->hlen.as<u32>(), B->hoff.as<u32>(), n2x, s, &entries));
    GHIP(hipStreamSynchronize(s));
    const u64 U = heads.total(), n_entries = entries.total();
    if (n_entries != (alive ? n_alive : n) || U == 0 || U > n_entries) return defect(broken);       // every (surviving) node lies on exactly one unitig
    // ---- walks and copy plan
    GHIP(B->offsets.ensure((U + 1) * 8)); GHIP(B->circ.ensure(U)); GHIP(B->length.ensure(U * 8)); GHIP(B->kc.ensure(U * 8));
    GHIP(B->node.ensure(n * 4)); GHIP(B->ori.ensure(n)); GHIP(B->src_read.ensure(n * 8)); GHIP(B->src_begin.ensure(n * 8)); GHIP(B->len.ensure(n * 4)); GHIP(B->rc.ensure(n));
    GHIP(B->dst.ensure(n * 8)); GHIP(B->ent_u.ensure(n * 4)); GHIP(B->pl64.ensure((n + 1) * 8)); GHIP(B->ab64.ensure((n + 1) * 8)); GHIP(B->gs.ensure((n + 1) * 8)); GHIP(B->ga.ensure((n + 1) * 8));
    EmitArgs ea; memset(&ea, 0, sizeof ea);
    ea.nd = nd; ea.n2x = n2x; ea.n_unitigs = U; ea.n_entries = n_entries; ea.P = P; ea.D = D; ea.flag = B->flag.as<u32>(); ea.uid = B->uid.as<u32>(); ea.hoff = B->hoff.as<u32>(); ea.cyc = cyc;
    ea.offsets = B->offsets.as<u64>(); ea.circular = B->circ.as<u8>(); ea.node = B->node.as<u32>(); ea.ori = B->ori.as<u8>(); ea.src_read = B->src_read.as<u64>();
    ea.src_begin = B->src_begin.as<u64>(); ea.len = B->len.as<u32>(); ea.rc = B->rc.as<u8>(); ea.ent_u = B->ent_u.as<u32>(); ea.pl64 = B->pl64.as<u64>(); ea.ab64 = B->ab64.as<u64>();
    hipLaunchKernelGGL(emit_kernel, dim3(gv), dim3(256), 0, s, ea);
    GHIP(excl_scan(B->tmp, B->pl64.as<u64>(), B->gs.as<u64>(), (size_t)(n_entries + 1), s));
    GHIP(excl_scan(B->tmp, B->ab64.as<u64>(), B->ga.as<u64>(), (size_t)(n_entries + 1), s));
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(n)), dim3(256), 0, s, n_entries, U, B->offsets.as<u64>(), B->ent_u.as<u32>(), B->gs.as<u64>(), B->ga.as<u64>(), B->dst.as<u64>(),
                       B->length.as<u64>(), B->kc.as<u64>());
    // ---- unitig edges: every edge record that is not an interior link, in source order
    u64 UE = 0;
    if (E) {
        GHIP(B->ekeep.ensure(E * 4)); GHIP(B->epos.ensure(E * 4));
        UedgeArgs ua; memset(&ua, 0, sizeof ua);
        ua.n_edges = E; ua.eu = B->eu.as<u32>(); ua.ev = B->ev.as<u32>(); ua.ov_in = ed.overlap; ua.nxt = B->nxt.as<u32>(); ua.P = P; ua.flag = B->flag.as<u32>(); ua.uid = B->uid.as<u32>();
        ua.length = B->length.as<u64>(); ua.keep = B->ekeep.as<u32>(); ua.pos = B->epos.as<u32>();
        hipLaunchKernelGGL(uedge_kernel<false>, dim3(grid_for(E)), dim3(256), 0, s, ua);
        GHIP(excl_scan(B->tmp, B->ekeep.as<u32>(), B->epos.as<u32>(), (size_t)E, s));
        GHIP(scan_total(B->ekeep.as<u32>(), B->epos.as<u32>(), (size_t)E, s, &uedges));
        GHIP(hipStreamSynchronize(s));
        UE = uedges.total();
        GHIP(B->un1.ensure(UE * 4 + 4)); GHIP(B->un2.ensure(UE * 4 + 4)); GHIP(B->uov.ensure(UE * 4 + 4)); GHIP(B->uo1.ensure(UE + 4)); GHIP(B->uo2.ensure(UE + 4));
        ua.n1 = B->un1.as<u32>(); ua.o1 = B->uo1.as<u8>(); ua.n2 = B->un2.as<u32>(); ua.o2 = B->uo2.as<u8>(); ua.ov = B->uov.as<u32>();
        if (UE) hipLaunchKernelGGL(uedge_kernel<true>, dim3(grid_for(E)), dim3(256), 0, s, ua);
    }
    GHIP(hipStreamSynchronize(s));
    GHIP(hipGetLastError());
    B->Pfin = P; B->Dfin = D; B->cycfin = cyc; B->n_arcs = 2 * E;
    out->n_unitigs = U; out->n_entries = n_entries; out->offsets = B->offsets.as<u64>(); out->node = B->node.as<u32>(); out->ori = B->ori.as<u8>();
    out->src_read = B->src_read.as<u64>(); out->src_begin = B->src_begin.as<u64>(); out->len = B->len.as<u32>(); out->revcomp = B->rc.as<u8>(); out->dst_offset = B->dst.as<u64>();
    out->length = B->length.as<u64>(); out->kc_sum = B->kc.as<u64>(); out->circular = B->circ.as<u8>(); out->n_rounds = rounds;
    out->edges.n = UE; out->edges.n1 = B->un1.as<u32>(); out->edges.o1 = B->uo1.as<u8>(); out->edges.n2 = B->un2.as<u32>(); out->edges.o2 = B->uo2.as<u8>(); out->edges.overlap = B->uov.as<u32>();
    return hipSuccess;
}

hipError_t build_unitigs(UnitigBuffers* B, const UnitigNodes& nd, const EdgeResult& ed, hipStream_t s, UnitigResult* out, int* broken) {
    return build_unitigs_masked(B, nd, ed, nullptr, 0, nullptr, s, out, broken);
}
