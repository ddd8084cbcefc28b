// transits.hip — the reads that span a unitig end to end, and which repeats they resolve, on the GPU (gfx950).  Definition: include/mdbg_hip.h
// (mdbg_graph_transits).  Input: the device arrays of a unitig list (unitigs.hip) with its edge records, the store's read offsets and minimizer -> read map, and
// the placement with records (placement.h): unitig_of_entry, the per-index place codes (code[t] = global entry | strand << 31 or NONE) and the edge records in
// key order, in the context's one placement scratch.  Vertices, pairs and record keys are packed as placement_dev.h says.
//
// A transit key (u, p, q) is sorted as the pair hi = u, lo = p << vb | q with vb the bits of a vertex of this list (2 * n_entries - 1); an index that ends no
// transit carries hi = n_unitigs, behind every key.  Two stable radix sorts, lo first and then hi, over no more bits than the list needs, give the definition's order.
//
//   (memset)            everything that is counted per unitig and per record <- 0
//   (placement_queue)   the counters and the map zeroed, entry_kernel, record_key_kernel, sort_pairs(rkey, rec): stable, so a key's run starts at its smallest
//                       record; place_windows_kernel: code[]
//   event_kernel        one thread per minimizer index t of the range classifies the pair code[t - 1] -> code[t]: LINK, CROSS (an explained crossing: its key is
//                       found in the sorted record keys) or BREAK (an unplaced window, a read's first index, a missing crossing); ev[t] = t + 1 unless LINK, else 0.
//                       The three counts are reduced per workgroup: one atomic each
//   (rocPRIM)           last = inclusive max-scan of ev: last[t - 1] - 1 is the last event in front of t, with no walk back along the read
//   transit_kernel      a CROSS whose last event is a CROSS closes a transit: the walk between them is checked against the definition's consequence (one unitig,
//                       one strand, m(u) windows from end to end; otherwise TX_DEFECT_SHAPE), the canonical key goes to (khi[t], klo[t]); one atomic per workgroup
//   (rocPRIM)           sort_pairs by lo, then by hi
//   head_kernel         flag[t] = 1 iff sorted key t is a key and differs from the one in front;  (rocPRIM) pos = exclusive scan of flag
//   row_kernel          a head unpacks its key into the columns at pos[t]; its count is the length of its run (binary search), its two records the first of the runs
//                       of the in-pair's and the out-pair's key.  passes[u] += count; a STRONG key (count >= min_support) counts for its unitig and for the
//                       direction of the record key it enters by and leaves by (cin, cout: two counters per record, at the key's smallest record)
//   ends_kernel         one thread per sorted record: SELF flags; the head of a key's run counts the key for n_in of the unitig its pair or its mirror enters at
//                       (u, 0, 0) and for n_out of the unitig either leaves at (u, m - 1, 0)
//   check_kernel        one thread per row: a strong key whose entrance or exit counter is not 1 shares p or q with another strong key: bad[u] = 1
//   verdict_kernel      one thread per unitig: the first rule that applies; n_repeats and n_resolved reduced per workgroup
//
// All sums are integers and every position comes from a sort or a scan: two calls give identical arrays.  No loop but the binary searches; the number of
// launches is fixed.  Per minimizer index of the range, beside the placement's 4: 31 bytes of temporaries (kind 1, the keys 12 and their second copy 12, which
// holds ev and last until the first sort writes it, flag 1, pos 4, the rows' direction bits 1) and 38 bytes of row columns, sized for the worst case because their
// number is known only on the device.  Per edge record, beside the placement's 24: cin and cout 16.  Per unitig 17 bytes of result and 6 of temporaries.
#include <cstring>

#include "transits.h"
#include "placement_dev.h"

struct TransitBuffers {
    Buf kind, klo, khi, klo2, khi2, flag, pos, dirs, tmp;   // per minimizer index (klo2 holds ev and last until the first sort)
    Buf zeroed;                                             // passes, n_in, n_out, strong, cin, cout, bad, self: one memset per call
    Buf verdict, unitig, iu, ie, is, ou, oe, os, irec, orec, count;      // the result (with passes, n_in, n_out of `zeroed`)
    StageTimer timer;
};

namespace {

enum : u8 { K_LINK = 0, K_BREAK = 1, K_CROSS = 2 };
enum : u8 { V_PLAIN = 0, V_RESOLVED = 1, V_UNRESOLVED = 2, V_SELF = 3 };      // MDBG_TRANSIT_* of include/mdbg_hip.h

struct TxArgs {
    u64 U, N, R; const u64* offsets; const u32* unitig_of_entry; const u32* n1; const u32* n2;
    const u64* rkey_sorted; const u32* rec_sorted;
    const u64* roff; const u32* mread; u64 i0, n_idx;
    const u32* code; u8* kind; u32* ev; u32* last; u64* klo; u32* khi; u8* flag; const u32* pos; u8* dirs; u64* counters;
    u32 vb; u64 min_support;
    u64* passes; u32* n_in; u32* n_out; u32* strong; u32* cin; u32* cout; u8* bad; u8* self; u8* verdict;
    u32* unitig; u32* iu; u32* ie; u8* is; u32* ou; u32* oe; u8* os; u32* irec; u32* orec; u64* count;
};

__global__ __launch_bounds__(256) void event_kernel(TxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[3] = {0, 0, 0};            // adjacent, links, explained crossings
    if (t < a.n_idx) {
        u8 kind = K_BREAK;
        const u32 c = a.code[t];
        u64 key = 0, p = 0;
        const PairKind pair = classify_pair(a.code, a.roff, a.mread, a.i0, t, c, a.unitig_of_entry, a.rkey_sorted, a.R, &key, &p);
        if (pair != PAIR_NONE) cnt[0] = 1;
        if (pair == PAIR_LINK) { cnt[1] = 1; kind = K_LINK; }
        else if (pair == PAIR_EXPLAINED) { cnt[2] = 1; kind = K_CROSS; }
        a.kind[t] = kind;
        a.ev[t] = kind == K_LINK ? 0u : (u32)t + 1u;
    }
    block_add<3>(cnt, a.counters, TX_C_ADJACENT);
}

__global__ __launch_bounds__(256) void transit_kernel(TxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[1] = {0};
    if (t < a.n_idx) {
        u64 lo = 0; u32 hi = (u32)a.U;
        const u32 pr = t > 0 && a.kind[t] == K_CROSS ? a.last[t - 1] : 0u;
        if (pr > 1 && a.kind[pr - 1] == K_CROSS) {                     // (a CROSS sits at an index > 0: pr - 2 is an index)
            const u64 t0 = pr - 1;
            const u32 cx = a.code[t0 - 1], cy = a.code[t0], cx2 = a.code[t - 1], cy2 = a.code[t];      // c = x -> y, c' = x' -> y'; all four placed
            const u32 ey = cy & ~RP_STRAND, ex2 = cx2 & ~RP_STRAND, s = cy >> 31;
            const u32 u = a.unitig_of_entry[ey];
            const u64 e_first = a.offsets[u], e_last = a.offsets[u + 1] - 1;
            const bool walks_all = a.unitig_of_entry[ex2] == u && cx2 >> 31 == s && t - t0 == e_last - e_first + 1 &&
                                   (s ? ey == e_last && ex2 == e_first : ey == e_first && ex2 == e_last);
            if (!walks_all) set_defect(a.counters, TX_DEFECT_SHAPE);
            else {
                const u32 p = s ? vertex_of_code(cy2) ^ 1u : vertex_of_code(cx), q = s ? vertex_of_code(cx) ^ 1u : vertex_of_code(cy2);
                lo = (u64)p << a.vb | q; hi = u; cnt[0] = 1;
            }
        }
        a.klo[t] = lo; a.khi[t] = hi;
    }
    block_add<1>(cnt, a.counters, TX_C_PASSES);
}

__global__ __launch_bounds__(256) void head_kernel(TxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u32 hi = a.khi[t];
    a.flag[t] = hi < a.U && (t == 0 || a.khi[t - 1] != hi || a.klo[t - 1] != a.klo[t]);
}

__global__ __launch_bounds__(256) void row_kernel(TxArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_idx) return;
    const u32 f = a.flag[t], d = a.pos[t];
    if (t == a.n_idx - 1) a.counters[TX_C_TRANSITS] = (u64)d + f;
    if (!f) return;
    const u32 u = a.khi[t];
    const u64 klo = a.klo[t];
    const u32 p = (u32)(klo >> a.vb), q = (u32)(klo & ((1ull << a.vb) - 1));
    u64 lo = t + 1, hi = a.n_idx;                          // the first position behind the key's run
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (a.khi[mid] == u && a.klo[mid] == klo) lo = mid + 1; else hi = mid; }
    const u64 count = lo - t;
    const u32 ep = p >> 1, eq = q >> 1;                    // (both came out of code[]: entries of the list)
    const u32 up = a.unitig_of_entry[ep], uq = a.unitig_of_entry[eq];
    const u32 v_first = (u32)(a.offsets[u] << 1), v_last = (u32)((a.offsets[u + 1] - 1) << 1);
    const u64 in_pair = pair_of(p, v_first), out_pair = pair_of(v_last, q);
    const u64 in_key = key_of_pair(p, v_first), out_key = key_of_pair(v_last, q);
    const u64 si = lower_bound(a.rkey_sorted, a.R, in_key), so = lower_bound(a.rkey_sorted, a.R, out_key);
    if (si >= a.R || so >= a.R || a.rkey_sorted[si] != in_key || a.rkey_sorted[so] != out_key) { set_defect(a.counters, TX_DEFECT_SHAPE); return; }
    const u32 ri = a.rec_sorted[si], ro = a.rec_sorted[so];
    const u32 di = in_pair != in_key, dout = out_pair != out_key;
    a.unitig[d] = u;
    a.iu[d] = up; a.ie[d] = (u32)(ep - a.offsets[up]); a.is[d] = (u8)(p & 1u);
    a.ou[d] = uq; a.oe[d] = (u32)(eq - a.offsets[uq]); a.os[d] = (u8)(q & 1u);
    a.irec[d] = ri; a.orec[d] = ro; a.count[d] = count; a.dirs[d] = (u8)(di | dout << 1);
    atomicAdd((unsigned long long*)(a.passes + u), (unsigned long long)count);
    if (count >= a.min_support) {
        atomicAdd(a.strong + u, 1u);
        atomicAdd(a.cin + (2 * (u64)ri + di), 1u);
        atomicAdd(a.cout + (2 * (u64)ro + dout), 1u);
    }
}

__global__ __launch_bounds__(256) void ends_kernel(TxArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.R) return;
    const u64 key = a.rkey_sorted[i];
    if (key == JX_NO_KEY) return;                          // (record_key_kernel has set JX_DEFECT_EDGE)
    const u32 r = a.rec_sorted[i];
    if (a.n1[r] == a.n2[r]) a.self[a.n1[r]] = 1;
    if (i > 0 && a.rkey_sorted[i - 1] == key) return;
    const u32 x = (u32)(key >> 32), y = (u32)key;
    if ((x >> 1) >= a.N || (y >> 1) >= a.N) { set_defect(a.counters, JX_DEFECT_EDGE); return; }
    const bool own_mirror = mirror_of_pair(key) == key;
    const u32 ux = a.unitig_of_entry[x >> 1], uy = a.unitig_of_entry[y >> 1];
    const u32 first_x = (u32)(a.offsets[ux] << 1), last_x = (u32)((a.offsets[ux + 1] - 1) << 1);
    const u32 first_y = (u32)(a.offsets[uy] << 1), last_y = (u32)((a.offsets[uy + 1] - 1) << 1);
    if (y == first_y) atomicAdd(a.n_in + uy, 1u);                            // the pair enters uy at (uy, 0, 0)
    if (!own_mirror && (x ^ 1u) == first_x) atomicAdd(a.n_in + ux, 1u);      // its mirror enters ux
    if (x == last_x) atomicAdd(a.n_out + ux, 1u);                            // the pair leaves ux at (ux, m - 1, 0)
    if (!own_mirror && (y ^ 1u) == last_y) atomicAdd(a.n_out + uy, 1u);      // its mirror leaves uy
}

__global__ __launch_bounds__(256) void check_kernel(TxArgs a) {
    const u64 d = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.n_idx || a.counters[RP_C_DEFECT] || d >= a.counters[TX_C_TRANSITS] || a.count[d] < a.min_support) return;      // (after a defect a row may not be written)
    const u32 dirs = a.dirs[d];
    if (a.irec[d] >= a.R || a.orec[d] >= a.R || a.unitig[d] >= a.U) { set_defect(a.counters, TX_DEFECT_SHAPE); return; }
    if (a.cin[2 * (u64)a.irec[d] + (dirs & 1u)] != 1u || a.cout[2 * (u64)a.orec[d] + (dirs >> 1)] != 1u) a.bad[a.unitig[d]] = 1;
}

__global__ __launch_bounds__(256) void verdict_kernel(TxArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 cnt[2] = {0, 0};               // repeats, resolved ones
    if (u < a.U) {
        const u32 ni = a.n_in[u], no = a.n_out[u];
        u8 v = V_PLAIN;
        if (ni >= 2 && no >= 2) {
            cnt[0] = 1;
            v = a.self[u] ? V_SELF : ni == no && a.strong[u] == ni && !a.bad[u] ? V_RESOLVED : V_UNRESOLVED;
            cnt[1] = v == V_RESOLVED;
        }
        a.verdict[u] = v;
    }
    block_add<2>(cnt, a.counters, TX_C_REPEATS);
}

u32 bits_of(u64 v) { u32 b = 1; while (b < 64 && (v >> b)) ++b; return b; }      // the bits that hold every value <= v

// the layout of `zeroed` for U unitigs and R records
struct Zeroed { size_t passes, n_in, n_out, strong, cin, cout, bad, self, bytes; };
Zeroed zeroed_of(u64 U, u64 R) {
    Zeroed z; size_t at = 0;
    z.passes = at; at += U * 8; z.n_in = at; at += U * 4; z.n_out = at; at += U * 4; z.strong = at; at += U * 4;
    z.cin = at; at += R * 8; z.cout = at; at += R * 8; z.bad = at; at += U; z.self = at; at += U;
    z.bytes = at + 8;
    return z;
}

TxArgs args_of(TransitBuffers* B, const PlacementView& V, const UnitigResult& ul, const ReadPathRange& rg, u64 min_support) {
    TxArgs a; memset(&a, 0, sizeof a);
    a.U = ul.n_unitigs; a.N = ul.n_entries; a.R = V.R; a.offsets = ul.offsets; a.unitig_of_entry = V.unitig_of_entry; a.n1 = ul.edges.n1; a.n2 = ul.edges.n2;
    a.rkey_sorted = V.rkey_sorted; a.rec_sorted = V.rec_sorted;
    a.roff = rg.roff; a.mread = rg.mread; a.i0 = rg.i0; a.n_idx = rg.i1 - rg.i0;
    a.code = V.code; a.kind = B->kind.as<u8>(); a.ev = B->klo2.as<u32>(); a.last = a.ev + a.n_idx + 1; a.klo = B->klo.as<u64>(); a.khi = B->khi.as<u32>();
    a.flag = B->flag.as<u8>(); a.pos = B->pos.as<u32>(); a.dirs = B->dirs.as<u8>(); a.counters = V.counters;
    a.vb = bits_of(2 * a.N - 1); a.min_support = min_support;
    const Zeroed z = zeroed_of(a.U, a.R);
    char* zp = B->zeroed.as<char>();
    a.passes = (u64*)(zp + z.passes); a.n_in = (u32*)(zp + z.n_in); a.n_out = (u32*)(zp + z.n_out); a.strong = (u32*)(zp + z.strong);
    a.cin = (u32*)(zp + z.cin); a.cout = (u32*)(zp + z.cout); a.bad = (u8*)(zp + z.bad); a.self = (u8*)(zp + z.self);
    a.verdict = B->verdict.as<u8>();
    a.unitig = B->unitig.as<u32>(); a.iu = B->iu.as<u32>(); a.ie = B->ie.as<u32>(); a.is = B->is.as<u8>(); a.ou = B->ou.as<u32>(); a.oe = B->oe.as<u32>(); a.os = B->os.as<u8>();
    a.irec = B->irec.as<u32>(); a.orec = B->orec.as<u32>(); a.count = B->count.as<u64>();
    return a;
}

}  // namespace

TransitBuffers* transit_buffers_create() { return new TransitBuffers(); }
void transit_buffers_destroy(TransitBuffers* b) { delete b; }

hipError_t transits_run(TransitBuffers* B, PlacementBuffers* P, const UnitigResult& ul, const u32* index, u64 n_rows, const ReadPathRange& rg, u64 min_support,
                        const WindowPlacer& placer, hipStream_t s, TransitResult* out, const OriginMap& om) {
    memset(out, 0, sizeof *out);
    const u64 U = ul.n_unitigs, R = ul.edges.n, n_idx = rg.i1 - rg.i0;
    if (U > ul.n_entries) return hipErrorInvalidValue;
    // every buffer first: growing one may wait for the device (graph_common.h), and nothing of this call is queued yet
    GHIP(placement_reserve(P, ul, n_rows, rg, true, om));
    const Zeroed z = zeroed_of(U, R);
    GHIP(B->zeroed.ensure(z.bytes)); GHIP(B->verdict.ensure(U + 4));
    GHIP(B->kind.ensure(n_idx + 4)); GHIP(B->klo.ensure(n_idx * 8 + 8)); GHIP(B->klo2.ensure(n_idx * 8 + 8)); GHIP(B->khi.ensure(n_idx * 4 + 4)); GHIP(B->khi2.ensure(n_idx * 4 + 4));
    GHIP(B->flag.ensure(n_idx + 4)); GHIP(B->pos.ensure(n_idx * 4 + 4)); GHIP(B->dirs.ensure(n_idx + 4));
    GHIP(B->unitig.ensure(n_idx * 4 + 4)); GHIP(B->iu.ensure(n_idx * 4 + 4)); GHIP(B->ie.ensure(n_idx * 4 + 4)); GHIP(B->is.ensure(n_idx + 4));
    GHIP(B->ou.ensure(n_idx * 4 + 4)); GHIP(B->oe.ensure(n_idx * 4 + 4)); GHIP(B->os.ensure(n_idx + 4));
    GHIP(B->irec.ensure(n_idx * 4 + 4)); GHIP(B->orec.ensure(n_idx * 4 + 4)); GHIP(B->count.ensure(n_idx * 8 + 8));
    if (n_idx) {   // the largest temporary of the stage's rocPRIM calls, so that `tmp` does not grow between them
        size_t tb = 0, most = 0;
        GHIP(rocprim::inclusive_scan(nullptr, most, B->klo2.as<u32>(), B->klo2.as<u32>(), (size_t)n_idx, rocprim::maximum<u32>(), s));
        GHIP(rocprim::radix_sort_pairs(nullptr, tb, B->klo.as<u64>(), B->klo2.as<u64>(), B->khi.as<u32>(), B->khi2.as<u32>(), (size_t)n_idx, 0u, 64u, s)); if (tb > most) most = tb;
        GHIP(rocprim::radix_sort_pairs(nullptr, tb, B->khi2.as<u32>(), B->khi.as<u32>(), B->klo2.as<u64>(), B->klo.as<u64>(), (size_t)n_idx, 0u, 32u, s)); if (tb > most) most = tb;
        GHIP(rocprim::exclusive_scan(nullptr, tb, B->flag.as<u8>(), B->pos.as<u32>(), 0u, (size_t)n_idx, rocprim::plus<u32>(), s)); if (tb > most) most = tb;
        GHIP(B->tmp.ensure(most + 256));
    }
    GHIP(B->timer.start(s));
    GHIP(hipMemsetAsync(B->zeroed.p, 0, z.bytes, s));
    PlacementView V;
    GHIP(placement_queue(P, ul, index, n_rows, rg, true, TX_C_N, placer, s, &V, om));
    const TxArgs a = args_of(B, V, ul, rg, min_support);
    if (a.n_idx) {
        const unsigned gi = grid_for(a.n_idx);
        const size_t n = (size_t)a.n_idx;
        hipLaunchKernelGGL(event_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(hipGetLastError());
        {
            size_t tb = 0;
            GHIP(rocprim::inclusive_scan(nullptr, tb, (const u32*)a.ev, a.last, n, rocprim::maximum<u32>(), s));
            GHIP(B->tmp.ensure(tb + 256));
            GHIP(rocprim::inclusive_scan(B->tmp.p, tb, (const u32*)a.ev, a.last, n, rocprim::maximum<u32>(), s));
        }
        hipLaunchKernelGGL(transit_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(hipGetLastError());
        GHIP(sort_pairs(B->tmp, (const u64*)a.klo, B->klo2.as<u64>(), (const u32*)a.khi, B->khi2.as<u32>(), n, 0u, 2 * a.vb, s));      // (ev and last are read: klo2 is free)
        GHIP(sort_pairs(B->tmp, (const u32*)B->khi2.as<u32>(), a.khi, (const u64*)B->klo2.as<u64>(), a.klo, n, 0u, bits_of(a.U), s));
        hipLaunchKernelGGL(head_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(excl_scan(B->tmp, (const u8*)a.flag, B->pos.as<u32>(), n, s));
        hipLaunchKernelGGL(row_kernel, dim3(gi), dim3(256), 0, s, a);
        GHIP(hipGetLastError());
    }
    if (a.R) hipLaunchKernelGGL(ends_kernel, dim3(grid_for(a.R)), dim3(256), 0, s, a);
    if (a.n_idx) hipLaunchKernelGGL(check_kernel, dim3(grid_for(a.n_idx)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(verdict_kernel, dim3(grid_for(a.U)), dim3(256), 0, s, a);
    GHIP(hipGetLastError());
    u64 h[PLACEMENT_COUNTERS] = {};
    GHIP(B->timer.stop_and_read(h, a.counters, (om.copies ? PLACEMENT_COUNTERS : TX_C_N) * sizeof(u64), s, &out->ms));
    out->ambiguous = h[NP_C_AMBIGUOUS]; out->resolved = h[NP_C_RESOLVED]; out->conflicts = h[NP_C_CONFLICTS]; out->unanchored = h[NP_C_UNANCHORED];
    out->defect = (u32)h[RP_C_DEFECT];
    if (out->defect) return hipSuccess;
    out->n_reads = rg.n_reads; out->n_crossings = h[TX_C_ADJACENT] - h[TX_C_LINKS]; out->n_explained = h[TX_C_EXPLAINED]; out->n_passes = h[TX_C_PASSES];
    out->n_transits = h[TX_C_TRANSITS]; out->n_unitigs = a.U; out->n_repeats = h[TX_C_REPEATS]; out->n_resolved = h[TX_C_RESOLVED];
    out->unitig = a.unitig; out->in_unitig = a.iu; out->in_entry = a.ie; out->in_strand = a.is; out->out_unitig = a.ou; out->out_entry = a.oe; out->out_strand = a.os;
    out->in_record = a.irec; out->out_record = a.orec; out->count = a.count;
    out->n_in = a.n_in; out->n_out = a.n_out; out->passes = a.passes; out->verdict = a.verdict;
    return hipSuccess;
}
