// finalize.hip — from the counting table to the node table (gfx950): marking first sightings and solid keys, the bitmaps and their popcount prefixes, the order and the
// rows of the nodes, the digest; the re-scan for nodes whose u16 abundance wrapped; the positions of remote sketches fetched on demand.
// Needs table.hip (Slot, TableArgs, find_slot, the key hash and comparison) and, for OWNL_MAX_WORLD, owner.hip.
#include "mdbg_dev.h"
// ---- finalize --------------------------------------------------------------------------------------
struct BatchTab {                 // batches sorted by first_ordinal (device copy)
    const u64* first_ordinal; const u32* n_reads; const u32* slot0; const u64* rank_base; u32 n;
    const u32* by_slot0; const u64* by_slot_first;   // the same batches sorted by slot0 (= call order): slot -> read ordinal
    const u64* by_m0; const u64* by_m0_rank;         // the batches sorted by position in the store: first minimizer index and its dense rank
    const u64* m0;                                   // in first_ordinal order: first minimizer index of the batch (dense index -> store index, claims_to_bits_kernel)
};
struct FinArgs {
    const Slot* tab; u64 cap; const u64* mx; u32 A; u32 casc; u32 k; u32 l;   // A: abundance filter; casc: ordinals tracked per slot (= A up to 8, else 1)
    const u64* mh; const u32* mpos; const u64* roff; const u32* mread; const u64* arena;
    BatchTab bt;
    u64* solid_list; u64* solid_count;       // compact list of solid slots (fin_mark -> fin_emit), any order
    u64* solid_dense;                        // dense ordered index of each listed slot's first sighting (-> its row, fin_order_kernel)
    const u64* n_solid_dev;                  // non-null: fin_order / fin_emit were launched for an ESTIMATED number of rows (their grid and the capacity of the
                                             // outputs) before the host knew the count: they take it from here and do nothing when it exceeds the estimate
    const u64* order;                        // non-null: slot of the node in row q (fin_emit then writes its rows in order: whole lines instead of
                                             // eleven scattered 2..8-byte stores per node)
    u64* o_row;                              // non-null: write node q at position q and its global row here (partitioned table)
    const u64* ath_override;                 // [Slot.pad - 1]: sighting whose metadata a node that wrapped its u16 abundance keeps (null: none)
    u64* bm_first; u64* bm_solid;            // bitmaps over dense ordered minimizer index
    u32 claims;                              // 1: by_first IS the insertion's claim map (TableArgs::claim) and dense index == store index: fin_mark only moves the marks of
                                             // keys whose first sighting is not their claimer (keys seen once — most — need nothing).  2 (round 6): the same map where the
                                             // dense order is NOT the store's (a partitioned table: the peers' regions lie between this rank's batches, batches out of
                                             // ordinal order): the map is indexed by STORE index, claims_to_bits_kernel turns it into the dense bitmaps
    u8* by_first; u8* by_solid;              // the same as one BYTE per index (zeroed): fin_mark sets bytes with plain stores — 3.9 M device-scope atomics on the
                                             // bitmaps were most of its time —, bytes_to_bits_kernel packs them into the bitmaps
    const u32* pre_first; const u32* pre_solid;   // exclusive popcount prefix per 64-bit word
    u64* sh_solid; u64* sh_wrapped; u64* sh_distinct;   // sharded counters (CTR_SHARDS u64 each)
    // outputs (device), node order = rank of first sighting among solid nodes
    u64* o_keys; u32* o_index; u16* o_abund; u32* o_seqlen; u16* o_shift; u64* o_shift_full;
    u64* o_src_read; u64* o_src_start; u64* o_src_end; u8* o_rev;
};

// ordinal -> (minimizer array index i, dense ordered index D)
__device__ inline void decode_ordinal(const FinArgs& F, u64 ord, u64& i, u64& D) {
    const u64 ro = ord >> WIN_BITS, win = ord & WIN_MASK;
    u32 lo = 0, hi = F.bt.n - 1;
    while (lo < hi) { const u32 mid = lo + ((hi - lo + 1) >> 1); if (F.bt.first_ordinal[mid] <= ro) lo = mid; else hi = mid - 1; }
    const u32 s0 = F.bt.slot0[lo];
    const u32 slot = s0 + (u32)(ro - F.bt.first_ordinal[lo]);
    i = F.roff[slot] + win;
    D = F.bt.rank_base[lo] + (i - F.roff[s0]);
}
// Dense ordered index of the minimizer at store index i (the window starting there): batches keep their order inside the store, so
// this needs neither the read map nor the read offsets.  Dense indices are ordered like the ordinals they stand for.
__device__ inline u64 dense_of_index(const FinArgs& F, u64 i) {
    u32 lo = 0, hi = F.bt.n - 1;
    while (lo < hi) { const u32 mid = lo + ((hi - lo + 1) >> 1); if (F.bt.by_m0[mid] <= i) lo = mid; else hi = mid - 1; }
    return F.bt.by_m0_rank[lo] + (i - F.bt.by_m0[lo]);
}
// ordinal of the occurrence that claimed the slot (it did no count / ordinal atomics)
__device__ inline u64 rep_ordinal(const FinArgs& F, u64 word) {
    const u32 rep = (u32)word;
    if (word & (1ull << 33)) return F.arena[(u64)rep * (F.k + 2) + F.k];
    const u32 slot = F.mread[rep];
    u32 lo = 0, hi = F.bt.n - 1;
    while (lo < hi) { const u32 mid = lo + ((hi - lo + 1) >> 1); if (F.bt.by_slot0[mid] <= slot) lo = mid; else hi = mid - 1; }
    return ((F.bt.by_slot_first[lo] + (slot - F.bt.by_slot0[lo])) << WIN_BITS) | ((u64)rep - F.roff[slot]);
}
struct SlotView { u32 count; u64 first, ath; bool solid; };
// merges the claimer back in: total count, smallest ordinal, A-th smallest ordinal (valid when count >= A)
// casc: number of smallest ordinals the table tracked (= A for A <= MDBG_CASCADE_MAX; 1 for larger A, whose A-th sighting comes from
// the re-scan of resolve_wrapped through ath_override)
__device__ inline SlotView slot_view(const Slot& e, u64 s, const u64* mx, u32 casc, u32 A_filter, u64 r, const u64* ath_override = nullptr) {
    SlotView v;
    v.count = e.count + 1u;
    v.first = r < e.m1 ? r : e.m1;
    const u32 A = casc;
    if (A == 1) v.ath = v.first;
    else {
        const u64 prev = A == 2 ? e.m1 : A == 3 ? e.m2 : mx[s * (A - 2) + (A - 4)];      // (A-1)-th smallest of the others
        const u64 last = A == 2 ? e.m2 : mx[s * (A - 2) + (A - 3)];                      // A-th smallest of the others
        v.ath = r < prev ? prev : (r < last ? r : last);
    }
    v.solid = A_filter == 1 || (u16)v.count >= (u16)A_filter;                             // src/main.rs:922-929 (u16 abundance)
    if (e.pad && ath_override) v.ath = ath_override[e.pad - 1];                            // see wrap_list_kernel
    return v;
}

// Finalize's marking pass for the byte-map mode (F.claims == 0: one byte map per bit, zeroed per finalize; the claim-map mode has fin_mark_claims_kernel).
// FIN_SPT slots per thread, all requested before the first is looked at: the kernel is a chain of dependent round trips (slot -> read
// offsets of the smallest ordinal -> bitmap atomic), and with one slot per thread its 9,700 workgroups went through it 19 deep
constexpr int FIN_SPT = 4;
__global__ __launch_bounds__(1024) void fin_mark_kernel(FinArgs F) {
    __shared__ u32 wcnt[16 * FIN_SPT];
    __shared__ u64 bbase;
    const u64 s0 = (u64)blockIdx.x * (1024 * FIN_SPT) + threadIdx.x;
    Slot e[FIN_SPT];
#pragma unroll
    for (int u = 0; u < FIN_SPT; ++u) { const u64 s = s0 + 1024ull * u; e[u].word = EMPTY; if (s < F.cap) e[u] = F.tab[s]; }
    u32 n_occ = 0, n_wrapped = 0; bool solid[FIN_SPT]; u64 m[FIN_SPT], dense[FIN_SPT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < FIN_SPT; ++u) {
        solid[u] = false;
        u64 D = 0;
        if (e[u].word != EMPTY) {
            const u32 count = e[u].count + 1u;
            ++n_occ; solid[u] = F.A == 1 || (u16)count >= (u16)F.A; n_wrapped += count >= 65536u ? 1u : 0u;          // as slot_view
            // first sighting: the claimer's window or the smallest ordinal the others pushed.  Most keys are seen once (sequencing
            // errors), and the claimer's dense index follows from `rep` alone: no read map / offset lookups for them
            if (e[u].word & (1ull << 33)) { u64 i; const u64 ro = rep_ordinal(F, e[u].word); decode_ordinal(F, ro < e[u].m1 ? ro : e[u].m1, i, D); }   // routed record
            else {
                D = dense_of_index(F, (u32)e[u].word);
                if (e[u].count) { u64 i, D1; decode_ordinal(F, e[u].m1, i, D1); if (D1 < D) D = D1; }
            }
            F.by_first[D] = 1;                       // (distinct keys have distinct first sightings: nobody else writes this byte)
            if (solid[u]) F.by_solid[D] = 1;
        }
        dense[u] = D;
        m[u] = __ballot(solid[u]);
        if (lane == 0) wcnt[16 * u + wv] = (u32)__popcll(m[u]);
    }
    for (int d = 32; d; d >>= 1) { n_occ += __shfl_down(n_occ, d, 64); n_wrapped += __shfl_down(n_wrapped, d, 64); }
    if (lane == 0) {
        if (n_occ) atomicAdd((unsigned long long*)ctr_shard(F.sh_distinct), (unsigned long long)n_occ);
        if (n_wrapped) atomicAdd((unsigned long long*)ctr_shard(F.sh_wrapped), (unsigned long long)n_wrapped);
    }
    // compact list of solid slots (any order): one allocation atomic per block
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 tot = 0;
        for (int i = 0; i < 16 * FIN_SPT; ++i) { const u32 c = wcnt[i]; wcnt[i] = tot; tot += c; }
        bbase = tot ? atomicAdd((unsigned long long*)F.solid_count, (unsigned long long)tot) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FIN_SPT; ++u)
        if (solid[u]) {
            const u64 j = bbase + wcnt[16 * u + wv] + __popcll(m[u] & ((1ull << lane) - 1));
            F.solid_list[j] = s0 + 1024ull * u; F.solid_dense[j] = dense[u];
        }
}
// The marking pass for the claim-map mode (F.claims), in two passes over the workgroup's 4,096 slots.  A slot needs more than a look only when its key was seen again
// (the first sighting may lie in front of the claimer: one scattered read, up to two scattered byte stores) or is solid (a row of the node table): 9 % of the human
// table's slots, which in fin_mark_kernel sit spread over every wave, so every wave waits for its few slow lanes on each of its four rounds.  Here the first pass
// only looks (word and count) and lists those slots in LDS; the second pass works the list off on full waves, and lists the solid ones once more for the ONE
// allocation atomic per workgroup (the counter is a single address: ~12 ns per atomic, serialised).
__global__ __launch_bounds__(1024) void fin_mark_claims_kernel(FinArgs F) {
    constexpr u32 SPAN = 1024 * FIN_SPT;
    __shared__ u16 lst[SPAN], sol_li[SPAN];
    __shared__ u32 sol_D[SPAN];
    __shared__ u32 n_lst, n_sol;
    __shared__ u64 bbase;
    const u64 b0 = (u64)blockIdx.x * SPAN;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { n_lst = 0; n_sol = 0; }
    __syncthreads();
    u32 n_occ = 0, n_wrapped = 0;
#pragma unroll
    for (int u = 0; u < FIN_SPT; ++u) {
        const u32 li = (u32)u * 1024u + threadIdx.x;
        const u64 s = b0 + li;
        bool slow = false;
        if (s < F.cap) {
            const u64 word = F.tab[s].word;
            if (word != EMPTY) {
                const u32 c0 = F.tab[s].count, count = c0 + 1u;
                ++n_occ; n_wrapped += count >= 65536u ? 1u : 0u;
                slow = c0 != 0 || F.A == 1 || (u16)count >= (u16)F.A;          // seen again, or solid (as slot_view)
            }
        }
        const u64 mk = __ballot(slow);
        u32 base = 0;
        if (lane == 0 && mk) base = atomicAdd(&n_lst, (u32)__popcll(mk));
        base = (u32)__shfl((int)base, 0, 64);
        if (slow) lst[base + (u32)__popcll(mk & ((1ull << lane) - 1ull))] = (u16)li;
    }
    for (int d = 32; d; d >>= 1) { n_occ += __shfl_down(n_occ, d, 64); n_wrapped += __shfl_down(n_wrapped, d, 64); }
    if (lane == 0) {
        if (n_occ) atomicAdd((unsigned long long*)ctr_shard(F.sh_distinct), (unsigned long long)n_occ);
        if (n_wrapped) atomicAdd((unsigned long long*)ctr_shard(F.sh_wrapped), (unsigned long long)n_wrapped);
    }
    __syncthreads();
    const u32 n = n_lst;
    for (u32 t0 = 0; t0 < n; t0 += 1024) {            // (the same trip count for every lane: ballots inside)
        const u32 t = t0 + threadIdx.x;
        bool solid = false; u32 li = 0; u64 D = 0;
        if (t < n) {
            li = lst[t];
            const Slot e = F.tab[b0 + li];
            const u32 count = e.count + 1u;
            solid = F.A == 1 || (u16)count >= (u16)F.A;
            // the claimer's byte is set already (insert_windows_kernel); a key seen again may have an earlier sighting: move the mark there.  ONE map in this mode: bit 0 =
            // first sighting, bit 1 = the key is solid
            const u64 ic = (u32)e.word;                                    // store index of the claimer; F.claims == 2: the map is indexed by store index, not by dense index
            const u64 Dc = F.claims == 2 ? dense_of_index(F, ic) : ic;
            u64 at = ic;
            D = Dc;
            if (e.count) { u64 i, D1; decode_ordinal(F, e.m1, i, D1); if (D1 < Dc) { D = D1; at = i; F.by_first[ic] = 0; } }
            // every listed slot (seen again, or solid) rewrites its byte: the solid bit is also CLEARED — solidity is (u16)count >= (u16)A, which turns false again when the
            // abundance wraps (count 65535 finalized as solid, more batches, count 65536 = u16 0, finalized again: round-5 advice; the byte-map path zeroes its maps per finalize)
            F.by_first[at] = solid ? 3 : 1;
        }
        const u64 mk = __ballot(solid);
        u32 base = 0;
        if (lane == 0 && mk) base = atomicAdd(&n_sol, (u32)__popcll(mk));
        base = (u32)__shfl((int)base, 0, 64);
        if (solid) { const u32 q = base + (u32)__popcll(mk & ((1ull << lane) - 1ull)); sol_li[q] = (u16)li; sol_D[q] = (u32)D; }
    }
    __syncthreads();
    const u32 ns = n_sol;
    if (threadIdx.x == 0) bbase = ns ? atomicAdd((unsigned long long*)F.solid_count, (unsigned long long)ns) : 0;
    __syncthreads();
    for (u32 t = threadIdx.x; t < ns; t += 1024) { F.solid_list[bbase + t] = b0 + sol_li[t]; F.solid_dense[bbase + t] = (u64)sol_D[t]; }
}
void launch_fin_mark(const FinArgs& F, hipStream_t s) {
    if (F.claims) { hipLaunchKernelGGL(fin_mark_claims_kernel, dim3((unsigned)((F.cap + 1024 * FIN_SPT - 1) / (1024 * FIN_SPT))), dim3(1024), 0, s, F); return; }
    hipLaunchKernelGGL(fin_mark_kernel, dim3((unsigned)((F.cap + 1024 * FIN_SPT - 1) / (1024 * FIN_SPT))), dim3(1024), 0, s, F);
}
// bitmap word w <- bit i = (byte 64 w + i != 0), for both maps; one thread per word (four 16-byte loads per map).  by1 == null: ONE map whose bytes hold bit 0 = first
// sighting, bit 1 = solid (the claim-map mode, fin_mark_claims_kernel).  Bits at or behind n_bits are cleared (the claim map's bytes behind the store's end are whatever
// the allocation holds: masked here instead of being zeroed by a fill in front of every finalize).  block_sum (non-null): the popcounts of the workgroup's 1,024 words of
// either bitmap — what popc_block_kernel would compute in a launch of its own: [blockIdx] and [n_blocks + blockIdx].
__global__ __launch_bounds__(1024) void bytes_to_bits_kernel(const u8* __restrict__ by0, const u8* __restrict__ by1, u64 n_words, u64 n_bits, u64* __restrict__ bm0, u64* __restrict__ bm1,
                                                             u32* __restrict__ block_sum, u32 n_blocks) {
    __shared__ u32 ws[2][16];
    const u64 w = (u64)blockIdx.x * 1024 + threadIdx.x;
    auto pack = [](const u8* p, u32 shift) -> u64 {
        u64 out = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = ((const uint4*)p)[q];
            const u32 x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) out |= (u64)(((((x[j] >> shift) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (16 * q + 4 * j);      // four bytes -> four bits, byte 0 lowest
        }
        return out;
    };
    u64 a = 0, b = 0;
    if (w < n_words) {
        a = pack(by0 + 64 * w, 0); b = by1 ? pack(by1 + 64 * w, 0) : pack(by0 + 64 * w, 1);
        if (64 * w + 64 > n_bits) { const u64 keep = 64 * w >= n_bits ? 0ull : (1ull << (n_bits - 64 * w)) - 1ull; a &= keep; b &= keep; }
        bm0[w] = a; bm1[w] = b;
    }
    if (!block_sum) return;
    u32 v0 = (u32)__popcll(a), v1 = (u32)__popcll(b);
    for (int d = 32; d; d >>= 1) { v0 += __shfl_down(v0, d, 64); v1 += __shfl_down(v1, d, 64); }
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = v0; ws[1][threadIdx.x >> 6] = v1; }
    __syncthreads();
    if (threadIdx.x < 2) { u32 t = 0; for (int i = 0; i < 16; ++i) t += ws[threadIdx.x][i]; block_sum[threadIdx.x * n_blocks + blockIdx.x] = t; }
}
// block_sum: null, or 2 * ceil(n_words / 1024) u32 (then launch_popc_prefix2 may skip its first kernel: have_block_sums)
void launch_bytes_to_bits(const u8* by0, const u8* by1, u64 n_words, u64 n_bits, u64* bm0, u64* bm1, u32* block_sum, hipStream_t s) {
    const u32 nb = (u32)((n_words + 1023) / 1024);
    if (n_words) hipLaunchKernelGGL(bytes_to_bits_kernel, dim3(nb), dim3(1024), 0, s, by0, by1, n_words, n_bits, bm0, bm1, block_sum, nb);
}
// F.claims == 2: the claim map is indexed by STORE index, the bitmaps by dense ordered index (the batches in first-ordinal order): one wave per 64 dense indices — lane l reads
// its bytes at its batch's place in the store (consecutive lanes read consecutive bytes except across a batch boundary).  ~1 byte read per resident minimizer; the per-block popcounts are left to popc_block_kernel (a partitioned table merges the bitmaps over the ranks first).
__global__ __launch_bounds__(256) void claims_to_bits_kernel(FinArgs F, u64 n_words, u64 n_bits, u64* __restrict__ bm0, u64* __restrict__ bm1) {
    // a lane takes EIGHT dense indices (one byte of either bitmap): one 8-byte load where the eight lie in one batch (all but the groups across a batch boundary), its eight
    // bits 0 and eight bits 1 gathered by a multiplication, stored as a byte: a wave reads 512 bytes and writes 64 + 64 per round.  (Until round 6 a lane read one byte and
    // two ballots made the words: 64 bytes per wave and load, 1.2 ms of a rank-of-eight's finalize, which runs over the WHOLE index space.)
    u32 bi = 0; u64 lo = 0, hi = 0, m0 = 0;                                    // the batch [lo, hi) of dense indices the lane looked at last
    auto locate = [&](u64 D) {
        if (D >= lo && D < hi) return;
        u32 a = 0, z = F.bt.n - 1;
        while (a < z) { const u32 mid = a + ((z - a + 1) >> 1); if (F.bt.rank_base[mid] <= D) a = mid; else z = mid - 1; }
        bi = a; lo = F.bt.rank_base[bi]; hi = bi + 1 < F.bt.n ? F.bt.rank_base[bi + 1] : n_bits; m0 = F.bt.m0[bi];
        // (batches without a minimizer share their rank base with the batch behind them: the search ends on the last of them, whose range [lo, hi) holds D)
    };
    const u64 n_groups = n_words * 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const u64 g = ((u64)blockIdx.x * 4 + u) * 256 + threadIdx.x;          // (consecutive lanes: consecutive groups)
        if (g >= n_groups) break;
        const u64 D = 8 * g;
        u64 x = 0;
        if (D < n_bits) {
            locate(D);
            if (D + 8 <= hi) {                          // eight bytes at any alignment: the two aligned words around them (the second one is the next lane's first: a hit)
                const u8* const p = F.by_first + m0 + (D - lo);
                const u32 o = (u32)((uintptr_t)p & 7u) * 8u;
                const u64* const q = (const u64*)(p - (o >> 3));
                x = q[0];
                if (o) x = (x >> o) | (q[1] << (64u - o));
            }
            else for (u32 t = 0; t < 8 && D + t < n_bits; ++t) { locate(D + t); x |= (u64)F.by_first[m0 + (D + t - lo)] << (8 * t); }
        }
        ((u8*)bm0)[g] = (u8)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
        ((u8*)bm1)[g] = (u8)((((x >> 1) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
    }
}
void launch_claims_to_bits(const FinArgs& F, u64 n_words, u64 n_bits, u64* bm0, u64* bm1, hipStream_t s) {
    if (n_words) hipLaunchKernelGGL(claims_to_bits_kernel, dim3((unsigned)((n_words * 8 + 1023) / 1024)), dim3(256), 0, s, F, n_words, n_bits, bm0, bm1);
}
// exclusive prefix of popcounts over 64-bit words, for the two finalize bitmaps at once: pre[w] = sum_{v<w} popc(bm[v]).  Block sums, scan
// of the block sums, per-word prefix — and with at most 1024 blocks (64 M bits) the last kernel adds up the sums in front of its block
// itself: two launches for both bitmaps where there were six (small kernels in a row cost ~5 us each on the device, more on the host)
__global__ __launch_bounds__(1024) void popc_block_kernel(const u64* __restrict__ bm0, const u64* __restrict__ bm1, u64 n_words, u32* __restrict__ block_sum, u32 n_blocks) {
    __shared__ u32 ws[2][16];
    const u64 w = (u64)blockIdx.x * 1024 + threadIdx.x;
    u32 v0 = w < n_words ? __popcll(bm0[w]) : 0, v1 = w < n_words ? __popcll(bm1[w]) : 0;
    for (int d = 32; d; d >>= 1) { v0 += __shfl_down(v0, d, 64); v1 += __shfl_down(v1, d, 64); }
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = v0; ws[1][threadIdx.x >> 6] = v1; }
    __syncthreads();
    if (threadIdx.x < 2) { u32 t = 0; for (int i = 0; i < 16; ++i) t += ws[threadIdx.x][i]; block_sum[threadIdx.x * n_blocks + blockIdx.x] = t; }
}
__global__ __launch_bounds__(1024) void popc_scan_blocks_kernel(u32* __restrict__ block_sum_all, u32 n_blocks) {
    __shared__ u32 ws[16]; __shared__ u32 run;
    u32* const block_sum = block_sum_all + (size_t)blockIdx.x * n_blocks;        // one workgroup per bitmap
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) run = 0;
    __syncthreads();
    for (u32 i0 = 0; i0 < n_blocks; i0 += 1024) {
        const u32 i = i0 + tid;
        const u32 v = i < n_blocks ? block_sum[i] : 0;
        const u32 inc = wave_incl_scan(v);
        if (lane == 63) ws[wv] = inc;
        __syncthreads();
        u32 b = run, tot = 0;
        for (int q = 0; q < 16; ++q) { if (q < wv) b += ws[q]; tot += ws[q]; }
        if (i < n_blocks) block_sum[i] = b + inc - v;
        __syncthreads();
        if (tid == 0) run += tot;
        __syncthreads();
    }
}
// self_base: block_sum holds the plain sums (no scan kernel ran; n_blocks <= 1024)
__global__ __launch_bounds__(1024) void popc_prefix_kernel(const u64* __restrict__ bm0, const u64* __restrict__ bm1, u64 n_words, const u32* __restrict__ block_sum, u32 n_blocks,
                                                           u32 self_base, u32* __restrict__ pre0, u32* __restrict__ pre1) {
    __shared__ u32 ws[2][16], bs[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 w = (u64)blockIdx.x * 1024 + tid;
    const u32 v0 = w < n_words ? __popcll(bm0[w]) : 0, v1 = w < n_words ? __popcll(bm1[w]) : 0;
    const u32 i0 = wave_incl_scan(v0), i1 = wave_incl_scan(v1);
    u32 s0 = 0, s1 = 0;
    if (self_base) {
        if ((u32)tid < blockIdx.x) { s0 = block_sum[tid]; s1 = block_sum[n_blocks + tid]; }
        for (int d = 32; d; d >>= 1) { s0 += __shfl_down(s0, d, 64); s1 += __shfl_down(s1, d, 64); }
    }
    if (lane == 63) { ws[0][wv] = i0; ws[1][wv] = i1; }
    if (lane == 0) { bs[0][wv] = s0; bs[1][wv] = s1; }
    __syncthreads();
    u32 b0, b1;
    if (self_base) { b0 = 0; b1 = 0; for (int q = 0; q < 16; ++q) { b0 += bs[0][q]; b1 += bs[1][q]; } }
    else { b0 = block_sum[blockIdx.x]; b1 = block_sum[n_blocks + blockIdx.x]; }
    for (int q = 0; q < wv; ++q) { b0 += ws[0][q]; b1 += ws[1][q]; }
    if (w < n_words) { pre0[w] = b0 + i0 - v0; pre1[w] = b1 + i1 - v1; }
}
// block_tmp: 2 * ceil(n_words / 1024) u32
// have_block_sums: block_tmp holds the plain per-block popcounts already (launch_bytes_to_bits wrote them with the bitmaps)
void launch_popc_prefix2(const u64* bm0, const u64* bm1, u64 n_words, u32* block_tmp, u32* pre0, u32* pre1, hipStream_t s, bool have_block_sums = false) {
    if (!n_words) return;
    const u32 nb = (u32)((n_words + 1023) / 1024);
    const u32 self_base = nb <= 1024 ? 1u : 0u;
    if (!have_block_sums) hipLaunchKernelGGL(popc_block_kernel, dim3(nb), dim3(1024), 0, s, bm0, bm1, n_words, block_tmp, nb);
    if (!self_base) hipLaunchKernelGGL(popc_scan_blocks_kernel, dim3(2), dim3(1024), 0, s, block_tmp, nb);
    hipLaunchKernelGGL(popc_prefix_kernel, dim3(nb), dim3(1024), 0, s, bm0, bm1, n_words, block_tmp, nb, self_base, pre0, pre1);
}
// out[0], out[1] = bits set in the two bitmaps (last prefix + popcount of the last word)
__global__ void bitmap_totals_kernel(const u64* __restrict__ bm0, const u32* __restrict__ pre0, const u64* __restrict__ bm1, const u32* __restrict__ pre1, u64 n_words, u64* __restrict__ out) {
    if (threadIdx.x == 0) out[0] = n_words ? (u64)pre0[n_words - 1] + (u64)__popcll(bm0[n_words - 1]) : 0;
    if (threadIdx.x == 1) out[1] = n_words ? (u64)pre1[n_words - 1] + (u64)__popcll(bm1[n_words - 1]) : 0;
}
void launch_bitmap_totals(const u64* bm0, const u32* pre0, const u64* bm1, const u32* pre1, u64 n_words, u64* out, hipStream_t s) {
    hipLaunchKernelGGL(bitmap_totals_kernel, dim3(1), dim3(64), 0, s, bm0, pre0, bm1, pre1, n_words, out);
}
// row of every listed solid slot (rank of its first sighting among the solid ones) -> order[row] = slot
__global__ __launch_bounds__(256) void fin_order_kernel(FinArgs F, u64 n_solid, u64* __restrict__ order) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (F.n_solid_dev) { const u64 n = *F.n_solid_dev; if (n > n_solid) return; n_solid = n; }      // (n_solid: the estimate the launch was sized for)
    if (q >= n_solid) return;
    const u64 D = F.solid_dense[q];
    order[F.pre_solid[D >> 6] + __popcll(F.bm_solid[D >> 6] & ((1ull << (D & 63)) - 1))] = F.solid_list[q];
}
void launch_fin_order(const FinArgs& F, u64 n_solid, u64* order, hipStream_t s) {
    if (n_solid) hipLaunchKernelGGL(fin_order_kernel, dim3((unsigned)((n_solid + 255) / 256)), dim3(256), 0, s, F, n_solid, order);
}

// One thread per solid node for the scalar fields; the k key values of a workgroup's 256 nodes are then copied by
// the whole workgroup, consecutive lanes on consecutive values, so that every row of o_keys is written as one run.
__global__ __launch_bounds__(256) void fin_emit_kernel(FinArgs F, u64 n_solid) {
    __shared__ u64 sh_src[256];              // minimizer index of the A-th sighting | reversed << 63
    __shared__ u64 sh_row[256];
    const u64 q0 = (u64)blockIdx.x * 256, q = q0 + threadIdx.x;
    const u32 k = F.k;
    if (F.n_solid_dev) { const u64 n = *F.n_solid_dev; if (n > n_solid || q0 >= n) return; n_solid = n; }      // (uniform over the workgroup)
    if (q < n_solid) {
        const u64 s = F.order ? F.order[q] : F.solid_list[q];
        const Slot e = F.tab[s];
        const SlotView v = slot_view(e, s, F.mx, F.casc, F.A, rep_ordinal(F, e.word), F.ath_override);
        u64 i1, D; decode_ordinal(F, v.first, i1, D);
        const u64 below = (1ull << (D & 63)) - 1;
        const u64 row = F.pre_solid[D >> 6] + __popcll(F.bm_solid[D >> 6] & below);          // row of the node in index order
        const u64 n = F.o_row ? q : row;
        if (F.o_row) F.o_row[q] = row;
        F.o_index[n] = F.pre_first[D >> 6] + __popcll(F.bm_first[D >> 6] & below);           // NODE_INDEX order (main.rs:661)
        F.o_abund[n] = (u16)v.count;
        // the A-th sighting (main.rs:680-684): seqlen, shift and the sequence's origin
        const u64 oa = v.ath;
        u64 i, Da; decode_ordinal(F, oa, i, Da);
        const u64* w = F.mh + i; const u32* p = F.mpos + i;
        const bool rev = window_reversed(w, k);
        sh_src[threadIdx.x] = i | ((u64)rev << 63); sh_row[threadIdx.x] = n;
        const u64 first = p[1] - p[0], last = p[k - 1] - p[k - 2];                             // main.rs:769-776
        const u64 s0 = rev ? last : first, s1 = rev ? first : last;
        F.o_seqlen[n] = (u32)((u64)p[k - 1] + 1 - p[0] + 1);                                   // main.rs:778 (read_offsets.2)
        F.o_shift[2 * n] = (u16)s0; F.o_shift[2 * n + 1] = (u16)s1;                            // main.rs:675
        F.o_shift_full[2 * n] = s0; F.o_shift_full[2 * n + 1] = s1;
        F.o_src_read[n] = oa >> WIN_BITS; F.o_src_start[n] = p[0]; F.o_src_end[n] = (u64)p[k - 1] + F.l;
        F.o_rev[n] = rev ? 1 : 0;
    }
    __syncthreads();
    // the keys: one wavefront per node, lane j copies element j (contiguous on both sides, no index arithmetic per element)
    const u32 nodes = (u32)(n_solid - q0 < 256 ? n_solid - q0 : 256);
    const u32 lane = threadIdx.x & 63;
    // (EMIT_NB nodes per wave and round, loads before stores: one node at a time was one full round trip per node, 64 in a row per wave)
    constexpr int EMIT_NB = 8;
    for (u32 g0 = (threadIdx.x >> 6) * EMIT_NB; g0 < nodes; g0 += 4 * EMIT_NB) {
        for (u32 j = lane; j < k; j += 64) {
            u64 v[EMIT_NB];
#pragma unroll
            for (int u = 0; u < EMIT_NB; ++u) {
                const u64 src = sh_src[g0 + u < nodes ? g0 + u : nodes - 1];
                v[u] = F.mh[(src & ~(1ull << 63)) + ((src >> 63) ? k - 1 - j : j)];
            }
#pragma unroll
            for (int u = 0; u < EMIT_NB; ++u) if (g0 + u < nodes) F.o_keys[sh_row[g0 + u] * k + j] = v[u];
        }
    }
}
void launch_fin_emit(const FinArgs& F, u64 n_solid, hipStream_t s) {
    if (n_solid) hipLaunchKernelGGL(fin_emit_kernel, dim3((unsigned)((n_solid + 255) / 256)), dim3(256), 0, s, F, n_solid);
}

// order-free digest of a node table (include/mdbg_hip.h, mdbg_nodes_digest): one thread per node, the workgroup's sum and XOR go to out[0], out[1] with one atomic each
__global__ __launch_bounds__(256) void nodes_digest_kernel(const u64* __restrict__ keys, const u16* __restrict__ abund, u64 n, u32 k, unsigned long long* __restrict__ out) {
    __shared__ u64 ws[2][4];
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    u64 h = 0;
    if (q < n) {
        h = 0x243F6A8885A308D3ull ^ (u64)abund[q];
        const u64* kp = keys + q * k;
        for (u32 j = 0; j < k; ++j) h = fmix64(h ^ kp[j]);
    }
    u64 sm = h, xr = h;
    for (int d = 32; d; d >>= 1) { sm += __shfl_down(sm, d, 64); xr ^= __shfl_down(xr, d, 64); }
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = sm; ws[1][threadIdx.x >> 6] = xr; }
    __syncthreads();
    if (threadIdx.x == 0) { atomicAdd(&out[0], (unsigned long long)(ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3])); atomicXor(&out[1], (unsigned long long)(ws[1][0] ^ ws[1][1] ^ ws[1][2] ^ ws[1][3])); }
}
void launch_nodes_digest(const u64* keys, const u16* abund, u64 n, u32 k, u64* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(nodes_digest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, abund, n, k, (unsigned long long*)out);
}

// ---- nodes whose u16 abundance wrapped (src/main.rs:676-684) ------------------------------------------
// The reference refreshes seqlen / shift (and writes the .sequences line) whenever the abundance BEFORE the increment
// equals minabund - 1.  The abundance is a u16 that wraps in release builds, so for a k-min-mer seen c >= 65536 + A times
// the entry ends up describing sighting j* = A + 65536 * floor((c - A) / 65536), not the A-th.  The min-cascade of the
// table only knows the A smallest ordinals; for these (rare, extremely repetitive) keys the exact j*-th smallest ordinal is
// recovered here: list them (Slot.pad = rank + 1), re-scan the resident windows (or routed records) collecting the
// ordinals of exactly those keys, sort each list, pick element j* - 1.
// all_solid: minabund exceeds what the slots track (MDBG_CASCADE_MAX): EVERY solid node gets its j*-th sighting this way.
__global__ __launch_bounds__(256) void wrap_list_kernel(Slot* __restrict__ tab, u64 cap, u32 A, bool all_solid, u64* __restrict__ w_jstar, u32* __restrict__ w_count,
                                                        unsigned long long* __restrict__ counters /* [0] nodes, [1] occurrences */) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const u64 word = tab[s].word;
    if (word == EMPTY) return;
    const u32 count = tab[s].count + 1u;
    if (count < A || (!all_solid && count - A < 65536u) || !(A == 1 || (u16)count >= (u16)A)) {
        // not listed (any more): a rank left by an earlier finalize (finalize -> ingest -> finalize without reset, the node's u16 abundance
        // has wrapped below minabund meanwhile) would send the scan kernels to another node's segment or past the lists
        if (tab[s].pad) tab[s].pad = 0;
        return;
    }
    const u32 r = (u32)atomicAdd(&counters[0], 1ull);
    atomicAdd(&counters[1], (unsigned long long)count);
    w_count[r] = count; w_jstar[r] = (u64)A + 65536ull * ((count - A) / 65536u);
    tab[s].pad = r + 1;
}
void launch_wrap_list(Slot* tab, u64 cap, u32 A, bool all_solid, u64* w_jstar, u32* w_count, unsigned long long* counters, hipStream_t s) {
    hipLaunchKernelGGL(wrap_list_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, tab, cap, A, all_solid, w_jstar, w_count, counters);
}
static size_t wrap_scan_windows_lds(const TableArgs& T) { return (256 + T.ks.k) * sizeof(u64); }      // the 256 + k - 1 hashes a workgroup's windows cover (+ one)
__global__ __launch_bounds__(256) void wrap_scan_windows_kernel(TableArgs T, const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff,
                                                                u64 i0, u64 i1, u32 slot0, u64 first_ordinal, const u32* __restrict__ w_start,
                                                                u32* __restrict__ w_fill, u64* __restrict__ occ) {
    extern __shared__ u64 sh_keys[];
    const u32 k = T.ks.k;
    const u64 b0 = i0 + (u64)blockIdx.x * 256;
    const u64 lim = b0 + 256 + k - 1 < i1 ? b0 + 256 + k - 1 : i1;
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    const u64 i = b0 + threadIdx.x;
    bool active = i < i1;
    u64 ord = 0;
    if (active) {
        const u32 slot = mread[i];
        const u64 rs = roff[slot], re = roff[slot + 1];
        active = re - rs > k && i + k <= re && i - rs <= WIN_MASK;
        ord = ((first_ordinal + (slot - slot0)) << WIN_BITS) | (i - rs);
    }
    __syncthreads();
    if (!active) return;
    const u64* w = sh_keys + threadIdx.x;
    if (T.own_world > 1 && window_owner(w, k, OwnerSpec{T.own_world, T.own_thr}) != T.own_rank) return;
    const bool rev = window_reversed(w, k);
    const u64 s = find_slot(T, key_hash_window(w, k, rev), [&](u64 word) { return same_key_window(T.ks, word, w, rev); });
    if (s == ~0ull) return;
    const u32 pad = T.tab[s].pad;
    if (pad) occ[w_start[pad - 1] + atomicAdd(&w_fill[pad - 1], 1u)] = ord;
}
void launch_wrap_scan_windows(const TableArgs& T, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 slot0, u64 first_ordinal,
                              const u32* w_start, u32* w_fill, u64* occ, hipStream_t s) {
    if (i1 > i0) hipLaunchKernelGGL(wrap_scan_windows_kernel, dim3((unsigned)((i1 - i0 + 255) / 256)), dim3(256), wrap_scan_windows_lds(T), s, T, mh, mread, roff,
                                    i0, i1, slot0, first_ordinal, w_start, w_fill, occ);
}
// the same over the LISTED windows of a batch (a foreign sketch of which only the listed windows' hashes are resident)
__global__ __launch_bounds__(256) void wrap_scan_listed_kernel(TableArgs T, const u64* __restrict__ mh, const u64* __restrict__ roff, u64 m0, u64 m1, const u32* __restrict__ list, u64 n,
                                                               u32 slot0, u32 n_reads, u64 first_ordinal, const u32* __restrict__ w_start, u32* __restrict__ w_fill, u64* __restrict__ occ) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 k = T.ks.k;
    const uint2 e = ((const uint2*)list)[j];
    const u64 i = m0 + e.x; const u32 slot = slot0 + e.y;
    if (e.y >= n_reads || i + k > m1) return;
    const u64 rs = roff[slot], re = roff[slot + 1];
    if (!(i >= rs && re - rs > k && i + k <= re && i - rs <= WIN_MASK)) return;
    const u64* w = mh + i;
    if (window_owner(w, k, OwnerSpec{T.own_world, T.own_thr}) != T.own_rank) return;
    const bool rev = window_reversed(w, k);
    const u64 s = find_slot(T, key_hash_window(w, k, rev), [&](u64 word) { return same_key_window(T.ks, word, w, rev); });
    if (s == ~0ull) return;
    const u32 pad = T.tab[s].pad;
    if (pad) occ[w_start[pad - 1] + atomicAdd(&w_fill[pad - 1], 1u)] = ((first_ordinal + e.y) << WIN_BITS) | (i - rs);
}
void launch_wrap_scan_listed(const TableArgs& T, const u64* mh, const u64* roff, u64 m0, u64 m1, const u32* list, u64 n, u32 slot0, u32 n_reads, u64 first_ordinal,
                             const u32* w_start, u32* w_fill, u64* occ, hipStream_t s) {
    if (n) hipLaunchKernelGGL(wrap_scan_listed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, mh, roff, m0, m1, list, n, slot0, n_reads, first_ordinal, w_start, w_fill, occ);
}
__global__ __launch_bounds__(256) void wrap_scan_records_kernel(TableArgs T, u64 n_records, const u32* __restrict__ w_start, u32* __restrict__ w_fill, u64* __restrict__ occ) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    const u32 k = T.ks.k;
    const u64* key = T.ks.arena + r * (k + 2);
    const u64 s = find_slot(T, key[k + 1], [&](u64 word) { return same_key_window(T.ks, word, key, false); });
    if (s == ~0ull) return;
    const u32 pad = T.tab[s].pad;
    if (pad) occ[w_start[pad - 1] + atomicAdd(&w_fill[pad - 1], 1u)] = key[k];
}
void launch_wrap_scan_records(const TableArgs& T, u64 n_records, const u32* w_start, u32* w_fill, u64* occ, hipStream_t s) {
    if (n_records) hipLaunchKernelGGL(wrap_scan_records_kernel, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, s, T, n_records, w_start, w_fill, occ);
}
__global__ void wrap_pick_kernel(u32 n_w, const u32* __restrict__ w_start, const u64* __restrict__ w_jstar, const u64* __restrict__ sorted, u64* __restrict__ ath_override) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_w) ath_override[r] = sorted[w_start[r] + w_jstar[r] - 1];
}
void launch_wrap_pick(u32 n_w, const u32* w_start, const u64* w_jstar, const u64* sorted, u64* ath_override, hipStream_t s) {
    if (n_w) hipLaunchKernelGGL(wrap_pick_kernel, dim3((n_w + 255) / 256), dim3(256), 0, s, n_w, w_start, w_jstar, sorted, ath_override);
}

// ---- positions of remote sketches, fetched on demand (multi-GPU sketch exchange, include/mdbg_dist.h) ----------------------------------
// The ranks exchange HASHES only (8 of the 12 bytes per minimizer).  Raw positions are needed for one thing: seqlen / shift / origin of
// the A-th sighting of a solid node (fin_emit_kernel reads p[0], p[1], p[k-2], p[k-1] of that window), and only the rank that sketched
// the read has them.  Before fin_emit every rank lists, per sketching rank, the A-th-sighting ordinals of its solid nodes that lie in
// somebody else's reads (pos_query_kernel: count pass, then write pass), the sketching rank answers with the four positions
// (pos_answer_kernel, through its own batch tables), and the answers are written into the local position array at the window's own
// indices (pos_scatter_kernel) — fin_emit then runs unchanged.  A few MB per finalize instead of 4 bytes per minimizer per step.
struct PosQueryArgs {
    const u32* batch_src;          // [F.bt.n] sketching rank of every batch, in F.bt order (sorted by first ordinal)
    u32 me, world, pass;           // pass 0: counts[peer] += 1; pass 1: write at offs[peer] + fill[peer]++
    unsigned long long* counts; const u64* offs; unsigned long long* fill;
    u64* q_ord; u64* q_idx;        // the query (ordinal of the A-th sighting) and the local store index of that window
};
__device__ inline u32 batch_of_ordinal(const FinArgs& F, u64 ord) {
    const u64 ro = ord >> WIN_BITS;
    u32 lo = 0, hi = F.bt.n - 1;
    while (lo < hi) { const u32 mid = lo + ((hi - lo + 1) >> 1); if (F.bt.first_ordinal[mid] <= ro) lo = mid; else hi = mid - 1; }
    return lo;
}
// (Per-peer counts and slots go through LDS: one global atomic per peer and workgroup.  One per node on `world` addresses was 6 ms per finalize at 8
// ranks — same-address atomics serialise.)
__global__ __launch_bounds__(256) void pos_query_kernel(FinArgs F, u64 n_solid, PosQueryArgs Q) {
    __shared__ u32 cnt[OWNL_MAX_WORLD];
    __shared__ u64 base[OWNL_MAX_WORLD];
    if (threadIdx.x < OWNL_MAX_WORLD) cnt[threadIdx.x] = 0;
    __syncthreads();
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 src = 0xFFFFFFFFu, local = 0; u64 ath = 0;
    if (q < n_solid) {
        const u64 s = F.solid_list[q];
        const Slot e = F.tab[s];
        const SlotView v = slot_view(e, s, F.mx, F.casc, F.A, rep_ordinal(F, e.word), F.ath_override);
        ath = v.ath;
        src = Q.batch_src[batch_of_ordinal(F, ath)];
        if (src == Q.me || src >= Q.world || src >= OWNL_MAX_WORLD) src = 0xFFFFFFFFu;
        else local = atomicAdd(&cnt[src], 1u);
    }
    __syncthreads();
    if (threadIdx.x < Q.world && threadIdx.x < OWNL_MAX_WORLD && cnt[threadIdx.x]) {
        if (Q.pass == 0) atomicAdd(&Q.counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        else base[threadIdx.x] = atomicAdd(&Q.fill[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    }
    if (Q.pass == 0) return;
    __syncthreads();
    if (src == 0xFFFFFFFFu) return;
    const u64 at = Q.offs[src] + base[src] + local;
    u64 i, D; decode_ordinal(F, ath, i, D);
    Q.q_ord[at] = ath; Q.q_idx[at] = i;
}
void launch_pos_query(const FinArgs& F, u64 n_solid, const PosQueryArgs& Q, hipStream_t s) {
    if (n_solid) hipLaunchKernelGGL(pos_query_kernel, dim3((unsigned)((n_solid + 255) / 256)), dim3(256), 0, s, F, n_solid, Q);
}
// answers: {p[0], p[1], p[k-2], p[k-1]} of the window with the given ordinal in THIS rank's store; *bad counts ordinals that are not
// windows of a batch this rank sketched (a protocol error)
__global__ __launch_bounds__(256) void pos_answer_kernel(FinArgs F, const u64* __restrict__ ords, u64 n, const u32* __restrict__ batch_src, u32 me, const u64* __restrict__ batch_m1,
                                                         uint4* __restrict__ ans, unsigned long long* __restrict__ bad) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u64 ord = ords[q];
    const u32 b = batch_of_ordinal(F, ord);
    const u64 ro = ord >> WIN_BITS;
    uint4 a = make_uint4(0u, 0u, 0u, 0u);
    if (batch_src[b] != me || ro < F.bt.first_ordinal[b] || ro - F.bt.first_ordinal[b] >= F.bt.n_reads[b]) { atomicAdd(bad, 1ull); ans[q] = a; return; }
    u64 i, D; decode_ordinal(F, ord, i, D);
    if (i + F.k > batch_m1[b]) { atomicAdd(bad, 1ull); ans[q] = a; return; }
    const u32* p = F.mpos + i;
    ans[q] = make_uint4(p[0], p[1], p[F.k - 2], p[F.k - 1]);
}
void launch_pos_answer(const FinArgs& F, const u64* ords, u64 n, const u32* batch_src, u32 me, const u64* batch_m1, uint4* ans, unsigned long long* bad, hipStream_t s) {
    if (n) hipLaunchKernelGGL(pos_answer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, F, ords, n, batch_src, me, batch_m1, ans, bad);
}
__global__ __launch_bounds__(256) void pos_scatter_kernel(const u64* __restrict__ idx, const uint4* __restrict__ ans, u64 n, u32 k, u32* __restrict__ mpos) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u64 i = idx[q]; const uint4 a = ans[q];
    mpos[i] = a.x; mpos[i + 1] = a.y; mpos[i + k - 2] = a.z; mpos[i + k - 1] = a.w;      // (k = 2: the same two entries twice, same values)
}
void launch_pos_scatter(const u64* idx, const uint4* ans, u64 n, u32 k, u32* mpos, hipStream_t s) {
    if (n) hipLaunchKernelGGL(pos_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, ans, n, k, mpos);
}
