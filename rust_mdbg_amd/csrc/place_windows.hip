// place_windows.hip — where on the current unitig list does every resident window lie (gfx950)?  The hot kernel of the placement (placement.h) that every read-evidence
// stage starts with; the rest of the placement is placement.hip.  Needs table.hip (the key hash and comparison, the slot layout) and finalize.hip (FinArgs, the batch table, the bitmaps).
//
// A window's key is looked up in the counting table as query_windows_kernel does; a hit that passes the abundance filter is a ROW of the last finalize's node table,
// and which row follows from what that finalize left behind, without a second table over the node keys: the slot's first sighting (its claimer, or the smallest
// ordinal the later sightings pushed) has a dense ordered index D, and the row is the rank of D among the solid bits, pre_solid[D >> 6] + popc(bm_solid[D >> 6] & below)
// — the expression fin_emit_kernel numbered the rows with.  fin_setup is the only writer of the bitmaps, the prefixes and the batch table, and it ends the node table
// (Results::invalidate, results.inc) before it touches them, so they are intact whenever the caller's state checks pass.
#include "mdbg_dev.h"
#include "placement.h"

// find_slot with the walk bounded by the table's capacity: ~0 when the key is absent; *full <- true when every slot was visited
template <class EqFn>
__device__ inline u64 find_slot_bounded(const TableArgs& T, u64 h, EqFn same_key, bool* full) {
    const u64 fp = (h >> 34) & T.fp_mask;
    u64 s = home_slot(h, T.cap);
    for (u64 probes = 0; probes < T.cap; ++probes) {
        const u64 w = load_relaxed(&T.tab[s].word);
        if (w == EMPTY) return ~0ull;
        if ((w >> 34) == fp && same_key(w)) return s;
        s = s + 1 == T.cap ? 0 : s + 1;
    }
    *full = true;
    return ~0ull;
}

constexpr int PW_SPAN = 1024;      // minimizer indices per workgroup, four per lane
// the kernel's dynamic LDS: the PW_SPAN + k - 1 hashes a workgroup's windows cover (+ one)
static size_t place_windows_lds(const TableArgs& T) { return ((size_t)PW_SPAN + T.ks.k) * sizeof(u64); }
// COPIES: the list holds copies (P.mult is set): a row that belongs to two or more entries gives the ambiguous code row | RP_AMBIGUOUS | rev << 31, which
// resolve_kernel (placement.hip) settles; such a window is not counted as placed here.  Everything else is the plain instantiation's.
template <bool COPIES>
__global__ __launch_bounds__(256) void place_windows_kernel(TableArgs T, FinArgs F, u64 fin_words, ReadPathPlan P, const u64* __restrict__ mh, const u32* __restrict__ mread,
                                                            const u64* __restrict__ roff, u64 i0, u64 i1) {
    extern __shared__ u64 sh_keys[];
    __shared__ u32 wsum[2][4];
    const u32 k = T.ks.k;
    const u64 b0 = i0 + (u64)blockIdx.x * PW_SPAN;
    const u64 lim = b0 + PW_SPAN + k - 1 < i1 ? b0 + PW_SPAN + k - 1 : i1;      // (the range ends where a read ends: no window of it reaches past i1)
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    __syncthreads();
    u32 n_win = 0, n_placed = 0, defect = 0;
#pragma unroll
    for (int u = 0; u < PW_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        const u64 i = b0 + li;
        if (i >= i1) break;
        u32 code = RP_NONE;
        const u32 slot = mread[i];
        const u64 rs = roff[slot], re = roff[slot + 1];
        if (re - rs > k && i + k <= re) {                                       // src/main.rs:756-759: a window starts here
            ++n_win;
            const u64* w = sh_keys + li;
            const bool rev = window_reversed(w, k);
            bool full = false;
            const u64 s = T.cap ? find_slot_bounded(T, key_hash_window(w, k, rev), [&](u64 word) { return same_key_window(T.ks, word, w, rev); }, &full) : ~0ull;
            if (full) defect |= RP_DEFECT_PROBE;
            if (s != ~0ull) {
                const u64 word = T.tab[s].word;
                const u32 others = T.tab[s].count, count = others + 1u;
                if (F.A == 1 || (u16)count >= (u16)F.A) {                      // a row of the node table: dbg_nodes.retain (main.rs:927), u16 abundance
                    u64 D = ~0ull;
                    if (!(word & (1ull << 33))) {                              // (a routed record: not on a context this stage accepts)
                        D = dense_of_index(F, (u32)word);                      // first sighting: the claimer's window or the smallest ordinal of the others (fin_mark_kernel)
                        if (others) { u64 i_, D1; decode_ordinal(F, T.tab[s].m1, i_, D1); if (D1 < D) D = D1; }
                    }
                    u64 row = ~0ull;
                    if ((D >> 6) < fin_words) {
                        const u64 bits = F.bm_solid[D >> 6];
                        if ((bits >> (D & 63)) & 1) row = F.pre_solid[D >> 6] + __popcll(bits & ((1ull << (D & 63)) - 1));
                    }
                    if (row < P.n_rows) {
                        const u32 e = P.entry_of_row[row];
                        if (COPIES && P.mult[row] >= 2u) code = (u32)row | RP_AMBIGUOUS | (rev ? RP_STRAND : 0u);
                        else if (e != RP_NONE) { code = e | ((rev != (P.ori[e] == '-')) ? RP_STRAND : 0u); ++n_placed; }
                    } else defect |= RP_DEFECT_ROW;
                }
            }
        }
        P.code[i - i0] = code;
    }
    // the workgroup's counts: one atomic each
    for (int d = 32; d; d >>= 1) { n_win += __shfl_down(n_win, d, 64); n_placed += __shfl_down(n_placed, d, 64); }
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = n_win; wsum[1][threadIdx.x >> 6] = n_placed; }
    if (defect) atomicOr((unsigned long long*)(P.counters + RP_C_DEFECT), (unsigned long long)defect);
    __syncthreads();
    if (threadIdx.x < 2) {
        const u32 t = wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
        if (t) atomicAdd((unsigned long long*)(P.counters + (threadIdx.x ? RP_C_PLACED : RP_C_WINDOWS)), (unsigned long long)t);
    }
}
void launch_place_windows(const TableArgs& T, const FinArgs& F, u64 fin_words, const ReadPathPlan& P, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, hipStream_t s) {
    if (i1 <= i0) return;
    const dim3 grid((unsigned)((i1 - i0 + PW_SPAN - 1) / PW_SPAN));
    if (P.mult) hipLaunchKernelGGL(place_windows_kernel<true>, grid, dim3(256), place_windows_lds(T), s, T, F, fin_words, P, mh, mread, roff, i0, i1);
    else hipLaunchKernelGGL(place_windows_kernel<false>, grid, dim3(256), place_windows_lds(T), s, T, F, fin_words, P, mh, mread, roff, i0, i1);
}
