// table.hip — k-min-mer windows, canonicalisation and the GPU-resident counting table (gfx950).
//
// Replaces the window loop of process_read_aux (rust-mdbg src/main.rs:756-781), KmerVec::normalize
// (src/kmer_vec.rs:34-39), add_kminmer's counting upsert on DashMap (src/main.rs:632-691, non-Bloom
// branch) and the abundance filter (src/main.rs:922-929).
//
// Table: open addressing, linear probing, 32-byte slots.  A slot is claimed with ONE 64-bit CAS on
//   word = fingerprint(30) | src(1) | rev(1) | rep(32)
// where `rep` points at a representative occurrence of the key (an index into the resident minimizer
// array, or into the routed-record arena when src=1) — the k*8-byte key itself is never copied.  A
// fingerprint hit is confirmed by comparing the full canonical key with the representative's, so the
// table is exact.  The occurrence that CLAIMS a slot costs exactly one atomic (the CAS): its ordinal
// (ordinal = read ordinal << 26 | window index) is recoverable from `rep`.  Every later occurrence of the key adds 1
// to `count` and offers its ordinal to the A smallest kept in m1, m2, mx[]; at finalize the claimer is merged back in
// (slot_view): the smallest ordinal gives DbgEntry.index (order of first sighting), the A-th gives the sighting whose
// seqlen/shift the reference stores, abundance = count + 1.
// The owner function and the owner codes (the multi-GPU partition of the key space) are defined here and not in owner.hip, which holds everything else about
// owners: insert_windows_kernel decides from them which windows are this rank's, and owner.hip's listed insertion needs upsert_wave in turn.
#include "mdbg_dev.h"

struct __attribute__((aligned(32))) Slot {
    u64 word;      // ~0 = empty
    u64 m1;        // smallest ordinal
    u64 m2;        // second smallest (A >= 2)
    u32 count;
    u32 pad;
};
constexpr u64 EMPTY = ~0ull;
constexpr u64 HMUL = 0x9E3779B97F4A7C15ull;

struct KeySrc {                   // where representative keys live
    const u64* mh;                // resident minimizer hashes (src = 0): key = mh[rep .. rep+k), orientation in the slot word
    const u64* arena;             // routed records (src = 1), k+2 u64 each: key = arena[rep*(k+2) .. +k), already canonical
    u32 k;
};

__device__ inline u64 load_relaxed(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// canonical element j of the key a slot word stands for
__device__ inline u64 rep_elem(const KeySrc& ks, u64 word, u32 j) {
    const u32 rep = (u32)word;
    if (word & (1ull << 33)) return ks.arena[(u64)rep * (ks.k + 2) + j];
    return (word & (1ull << 32)) ? ks.mh[(u64)rep + ks.k - 1 - j] : ks.mh[(u64)rep + j];
}

// KmerVec::normalize (src/kmer_vec.rs:34-39): true = the reversed vector is the canonical one (ties included)
__device__ inline bool window_reversed(const u64* __restrict__ w, u32 k) {
    for (u32 j = 0; j < k / 2 + 1 && j < k; ++j) {
        const u64 a = w[j], b = w[k - 1 - j];
        if (a < b) return false;
        if (a > b) return true;
    }
    return true;
}
// Hash of a canonical key given by an accessor elem(j): four independent multiply-xorshift chains over j mod 4 (the
// chain of one lane would otherwise be k dependent 64-bit multiplies), folded and finished with fmix64.
template <class ElemFn>
__device__ inline u64 key_hash_fn(ElemFn elem, u32 k) {
    u64 h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull, h2 = 0xA4093822299F31D0ull, h3 = 0x082EFA98EC4E6C89ull;
    u32 j = 0;
    for (; j + 4 <= k; j += 4) {
        h0 = (h0 ^ elem(j)) * HMUL;     h0 ^= h0 >> 29;
        h1 = (h1 ^ elem(j + 1)) * HMUL; h1 ^= h1 >> 29;
        h2 = (h2 ^ elem(j + 2)) * HMUL; h2 ^= h2 >> 29;
        h3 = (h3 ^ elem(j + 3)) * HMUL; h3 ^= h3 >> 29;
    }
    if (j < k) { h0 = (h0 ^ elem(j)) * HMUL; h0 ^= h0 >> 29; }
    if (j + 1 < k) { h1 = (h1 ^ elem(j + 1)) * HMUL; h1 ^= h1 >> 29; }
    if (j + 2 < k) { h2 = (h2 ^ elem(j + 2)) * HMUL; h2 ^= h2 >> 29; }
    return fmix64(h0 ^ rol64(h1, 17) ^ rol64(h2, 31) ^ rol64(h3, 47));
}
__device__ inline u64 key_hash_window(const u64* __restrict__ w, u32 k, bool rev) {
    return key_hash_fn([&](u32 j) { return rev ? w[k - 1 - j] : w[j]; }, k);
}
// The same hash of a window that lies in HBM, with the window's smallest value as a by-product: sixteen values per round trip (the loop of key_hash_fn fetches four, waits,
// mixes: nine dependent round trips at k = 35, and the owner check's loop another k) — the per-entry insertion of listed windows spent its time waiting on those chains.
__device__ inline u64 key_hash_window_hbm(const u64* __restrict__ w, u32 k, bool rev, u64& smallest) {
    u64 h[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
    const u64* const p = rev ? w + (k - 1) : w;
    const long st = rev ? -1 : 1;
    u64 mn = ~0ull;
    for (u32 j0 = 0; j0 < k; j0 += 16) {
        u64 v[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) { const u32 j = j0 + t < k ? j0 + t : k - 1; v[t] = p[st * (long)j]; }
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (j0 + t < k) { h[t & 3] = (h[t & 3] ^ v[t]) * HMUL; h[t & 3] ^= h[t & 3] >> 29; mn = v[t] < mn ? v[t] : mn; }      // (j0 is a multiple of 4: position j feeds chain j mod 4, as key_hash_fn)
    }
    smallest = mn;
    return fmix64(h[0] ^ rol64(h[1], 17) ^ rol64(h[2], 31) ^ rol64(h[3], 47));
}
__device__ inline u64 key_hash_canon(const u64* __restrict__ key, u32 k) {
    return key_hash_fn([&](u32 j) { return key[j]; }, k);
}

struct TableArgs {
    Slot* tab; u64 cap;           // number of slots (any value >= 1024)
    u64* mx;                      // [capacity][A-2] further minima when A > 2, else null
    u32 A;
    u64* n_distinct;              // device counter
    KeySrc ks;
    u32 own_world, own_rank;      // replicated-sketch mode: insert only windows owned by own_rank (own_world <= 1: all)
    const u64* own_thr;           // see OwnerSpec
    u32* probe_err;               // set when a probe sequence visited every slot: the table was sized from a wrong window count
    u64* own_inserted;            // sharded counter: owned windows actually inserted (checked against the senders' counts)
    u64 fp_mask;                  // 0x3FFFFFFF; MDBG_WEAK_FP (test hook) leaves two bits, so that most probes meet ANOTHER key behind their fingerprint
    unsigned long long* link_ctr; // non-null (MDBG_COUNT_LINKS): matches confirmed as links are counted here
    u32 no_chain;                 // 1: every fingerprint hit is confirmed by the full comparison (MDBG_NO_CHAIN; see insert_windows_kernel)
    u8* claim;                    // non-null: claim[i] <- 1 when the window starting at minimizer index i CLAIMED its slot (created the key), else 0 — written for every
                                  // index of the span, so the map needs no zeroing; finalize starts from it instead of marking every key's first sighting (fin_mark_kernel)
};

// Home slot of a key hash: range reduction by multiplication, so the capacity need not be a power of two.  It is fed
// from the LOW 40 bits of the hash: the high bits choose the owning rank in the routed mode (route.hip) and the
// fingerprint, and must stay independent of the position inside one rank's table.
__device__ inline u64 home_slot(u64 h, u64 cap) { return __umul64hi(h << 24, cap); }

// insert ordinal x into the slot's A smallest (exact whatever the other lanes do: every level is an atomicMin, a displaced value moves one level down)
__device__ inline void push_ordinal(const TableArgs& T, u64 s, u64 x) {
    Slot* e = T.tab + s;
    const u32 A = T.A;
    u64 carry = x;
    for (u32 lvl = 0; lvl < A && carry != EMPTY; ++lvl) {
        u64* m = lvl == 0 ? &e->m1 : lvl == 1 ? &e->m2 : &T.mx[s * (A - 2) + (lvl - 2)];
        const u64 old = atomicMin((unsigned long long*)m, (unsigned long long)carry);
        if (old > carry) carry = old;          // I displaced `old`; it moves one level down
    }
}
// A later occurrence (ordinal x) of the key in slot s: one more sighting, and x is offered to the slot's A smallest.  The one owner of what follows a confirmed match
// (the four insertion kernels, here and in owner.hip).
// Order: (1) `last`, the slot's current A-th smallest (m1, m2 or the last of mx[]), is loaded FIRST — the probe fetched that line a moment ago, it is still in the XCD's L2;
// (2) the cheap reject and, for an ordinal that passes, the atomicMin cascade; (3) the count, as the lane's LAST memory operation.  A device-scope atomic is executed at the
// memory side and drops the line from the L2, and one without a return value stays counted in vmcnt for its whole round trip (600 - 3,000 cycles): with the count in front
// (until round 6) the load of `last` was a certain L2 miss and the wait in front of the compare covered an atomic whose result nobody reads.
// Exact: m1, m2 and mx[] only ever decrease, so a value of `last` that is stale — from before another lane's update, or from this XCD's L2 — is larger than or equal to the
// true one.  It can only let an ordinal through to the cascade, which is exact on its own; it can never reject one that belongs.  The count is a sum: its place in the order
// does not change it, and nobody reads it before the kernel has ended.
__device__ inline void record_hit(const TableArgs& T, u64 s, u64 x) {
    Slot* e = T.tab + s;
    const u32 A = T.A;
    const u64* last = A == 1 ? &e->m1 : A == 2 ? &e->m2 : &T.mx[s * (A - 2) + (A - 3)];
    if (x <= load_relaxed(last)) push_ordinal(T, s, x);      // (else: x is larger than the A-th smallest — values only ever decrease)
    atomicAdd(&e->count, 1u);
}

// find-or-claim the slot of a key; same_key(word) = full comparison of my key with the representative a slot word names.
// upsert_slot_from: the same walk entered at slot s after `probes` slots have been looked at already (insert_windows_kernel's second stage).
template <class EqFn>
__device__ inline u64 upsert_slot_from(const TableArgs& T, u64 h, u64 myword_lo, EqFn same_key, bool& claimed, u64 s, u64 probes);
template <class EqFn>
__device__ inline u64 upsert_slot(const TableArgs& T, u64 h, u64 myword_lo, EqFn same_key, bool& claimed) {
    return upsert_slot_from(T, h, myword_lo, same_key, claimed, home_slot(h, T.cap), 0);
}
template <class EqFn>
__device__ inline u64 upsert_slot_from(const TableArgs& T, u64 h, u64 myword_lo, EqFn same_key, bool& claimed, u64 s, u64 probes) {
    claimed = false;
    const u64 fp = (h >> 34) & T.fp_mask;
    const u64 myword = (fp << 34) | myword_lo;
    for (; probes <= T.cap; ++probes) {
        u64 w = load_relaxed(&T.tab[s].word);      // (claiming without looking first — one round trip for a new key instead of two — is slower:
        if (w == EMPTY) {                          //  0.72 instead of 0.65 ms per 6.6 M windows; the kernel is bound by the rate of its atomics)
            const u64 old = atomicCAS((unsigned long long*)&T.tab[s].word, (unsigned long long)EMPTY, (unsigned long long)myword);
            if (old == EMPTY) { wave_agg_inc(T.n_distinct); claimed = true; return s; }
            w = old;
        }
        if ((w >> 34) == fp && same_key(w)) return s;
        s = s + 1 == T.cap ? 0 : s + 1;
    }
    *T.probe_err = 1;                          // table full: cannot happen when it was sized from the true number of windows
    return ~0ull;
}
// comparison of a key given as a contiguous run wl[0..k) (a window staged in LDS with orientation rev_mine, or a routed
// record's canonical key) with the representative in HBM: both are
// contiguous, so the representative is read 16 bytes per load, eight values per round trip; the last round overlaps.
typedef u64 u64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
__device__ inline bool same_key_window(const KeySrc& ks, u64 w, const u64* wl, bool rev_mine) {
    const u32 k = ks.k, rep = (u32)w;
    const u64* rp; bool cross;                // cross: rp[j] pairs with wl[k-1-j]
    if (w & (1ull << 33)) { rp = ks.arena + (u64)rep * (k + 2); cross = rev_mine; }
    else { rp = ks.mh + rep; cross = rev_mine != ((w & (1ull << 32)) != 0); }
    if (k < 8) {
        u64 diff = 0;
        for (u32 j = 0; j < k; ++j) diff |= rp[j] ^ wl[cross ? k - 1 - j : j];
        return !diff;
    }
    if (k >= 16) {
        // sixteen values per round trip (eight 16-byte loads in flight): k = 35 takes three dependent rounds instead of five
        for (u32 j = 0;; j += 16) {
            if (j + 16 > k) j = k - 16;
            u64x2_a8 a[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) a[t] = *(const u64x2_a8*)(rp + j + 2 * t);
            u64 diff = 0;
            if (!cross) {
                const u64* m = wl + j;
#pragma unroll
                for (int t = 0; t < 8; ++t) diff |= (a[t].x ^ m[2 * t]) | (a[t].y ^ m[2 * t + 1]);
            } else {
                const u64* m = wl + (k - 16 - j);      // m[15-t] pairs with rp[j+t]
#pragma unroll
                for (int t = 0; t < 8; ++t) diff |= (a[t].x ^ m[15 - 2 * t]) | (a[t].y ^ m[14 - 2 * t]);
            }
            if (diff) return false;
            if (j + 16 >= k) return true;
        }
    }
    for (u32 j = 0;; j += 8) {
        if (j + 8 > k) j = k - 8;
        const u64x2_a8 a0 = *(const u64x2_a8*)(rp + j), a1 = *(const u64x2_a8*)(rp + j + 2),
                       a2 = *(const u64x2_a8*)(rp + j + 4), a3 = *(const u64x2_a8*)(rp + j + 6);
        u64 diff;
        if (!cross) {
            const u64* m = wl + j;
            diff = (a0.x ^ m[0]) | (a0.y ^ m[1]) | (a1.x ^ m[2]) | (a1.y ^ m[3]) | (a2.x ^ m[4]) | (a2.y ^ m[5]) | (a3.x ^ m[6]) | (a3.y ^ m[7]);
        } else {
            const u64* m = wl + (k - 8 - j);   // m[7-t] pairs with rp[j+t]
            diff = (a0.x ^ m[7]) | (a0.y ^ m[6]) | (a1.x ^ m[5]) | (a1.y ^ m[4]) | (a2.x ^ m[3]) | (a2.y ^ m[2]) | (a3.x ^ m[1]) | (a3.y ^ m[0]);
        }
        if (diff) return false;
        if (j + 8 >= k) return true;
    }
}

// Owner of a k-min-mer in the replicated-sketch multi-GPU mode: a function of the SMALLEST of its k minimizer hashes (the same for the key
// and its reverse).  Consecutive windows of a read share their smallest hash for (k + 1) / 2 steps on average, so a rank's windows come in
// runs: a run of r windows needs r + k - 1 hashes of the read and nothing else of it, which is what the sketching rank ships to the owner
// (mdbg_dist, "segments") — a few hashes per window instead of the whole sketch to every rank.  (Round 2 hashed both ends and the middle: an
// O(1) function, but neighbouring windows went to unrelated ranks and every rank needed every hash.)
// The smallest of k values that are uniform on [0, bound] (the selected minimizers' hashes) has the distribution function
// 1 - (1 - v / bound)^k, and a minimizer that is small is the smallest of MANY windows: hashing the value to a rank left one of eight
// ranks with 43 % more nodes than the mean (l = 12: the few hundred smallest l-mer hashes carry most windows).  Cutting [0, 1) of that
// distribution function into `world` equal parts gives every rank the same expected share whatever the weights: 1.05 instead of 1.43.
// Owner parameters in device memory (u64 units): [0] = bin multiplier (0: no table), [1 .. 64) thresholds, ascending: rank r owns the minima v with
// thr[r - 1] <= v < thr[r]; from [64]: OWNER_BINS bytes, the owner of every bin of the value range (bin = mulhi64(v, multiplier)) — a MEASURED
// assignment: the multi-GPU layer counts the window minima of its first round per bin, sums the counts over the ranks and deals the bins out
// heaviest first to the least loaded rank (dist_api.inc, build_owner_table), so that a handful of very frequent small hashes (l = 12: ~700 distinct
// homopolymer-compressed 12-mers under the threshold, the smallest one the minimum of 5 % of all windows) cannot leave one rank with 20 % more
// than its share.  Neighbouring windows still share their owner (it is still a function of the smallest hash alone).
constexpr u32 OWNER_BINS = 65536, OWNER_THR_AT = 1, OWNER_TAB_AT = 64, OWNER_PARAM_WORDS = OWNER_TAB_AT + OWNER_BINS / 8;
struct OwnerSpec { u32 world; const u64* thr; };      // thr: the block above (null: hash the value)
__device__ inline u32 owner_of_min(u64 m, u32 k, OwnerSpec os);
__device__ inline u32 window_owner(const u64* __restrict__ w, u32 k, OwnerSpec os) {
    if (os.world <= 1) return 0;
    u64 m = w[0];
    for (u32 j = 1; j < k; ++j) { const u64 x = w[j]; m = x < m ? x : m; }
    return owner_of_min(m, k, os);
}
__device__ inline u32 owner_of_min(u64 m, u32 k, OwnerSpec os) {
    (void)k;
    if (os.world <= 1) return 0;
    if (!os.thr) return (u32)__umul64hi(fmix64(m), (u64)os.world);
    const u64 mul = os.thr[0];
    if (mul) {
        const u64 bin = __umul64hi(m, mul);
        const u32 o = ((const u8*)(os.thr + OWNER_TAB_AT))[bin < OWNER_BINS ? bin : OWNER_BINS - 1];
        return o < os.world ? o : os.world - 1;
    }
    const u64* const thr = os.thr + OWNER_THR_AT;
    u32 lo = 0, hi = os.world - 1;                  // number of thresholds <= m
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (thr[mid] <= m) lo = mid + 1; else hi = mid; }
    return lo;
}

// ---- owner codes --------------------------------------------------------------------------------------------------------------------------------------------
// A window's owner is a function of the SMALLEST of its k hashes, and both owner functions with parameters (OwnerSpec::thr) are monotone in that value up to a final table
// lookup: bin(v) = min(mulhi64(v, mul), OWNER_BINS - 1) for the measured table, rank(v) = number of thresholds <= v without one.  So
// min over the window of code(v) = code(min over the window of v), and the sliding minimum runs on 16-bit CODES: the values are turned into codes once, the doubling rounds
// (min over 2, 4, ... p <= k codes; a window of k is two overlapping stretches of p) move 2 bytes per element instead of 8 — round 3 ran them on the u64 hashes in 33 KB
// of LDS per workgroup, and a kernel that also needs the hashes themselves (the insertion) could not afford them at all.  (No parameters — the value is hashed to a rank —
// is not monotone: callers fall back to window_owner.)
struct OwnerCodes { u64 mul; const u64* thr; u32 world; };      // mul != 0: bins of the measured table; else threshold ranks
__device__ inline OwnerCodes owner_codes_of(OwnerSpec os) { OwnerCodes c; c.thr = os.thr; c.world = os.world; c.mul = os.thr ? os.thr[0] : 0; return c; }
__device__ inline u16 owner_code(u64 v, const OwnerCodes& c) {
    if (c.mul) { const u64 bin = __umul64hi(v, c.mul); return (u16)(bin < OWNER_BINS ? bin : OWNER_BINS - 1); }
    const u64* const thr = c.thr + OWNER_THR_AT;
    u32 lo = 0, hi = c.world - 1;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (thr[mid] <= v) lo = mid + 1; else hi = mid; }
    return (u16)lo;
}
__device__ inline u32 owner_of_code(u16 code, const OwnerCodes& c) {
    if (!c.mul) return code;
    const u32 o = ((const u8*)(c.thr + OWNER_TAB_AT))[code];
    return o < c.world ? o : c.world - 1;
}
// a, b: two LDS arrays of nv u16; value(t): the hash at span position t, valid(t): it exists.  Returns M with M[t] = smallest code among the p values from t on (p = the
// largest power of two <= k): the code of the window starting at span position li is min(M[li], M[li + k - p]).  All 256 threads call it.
template <class ValueFn, class ValidFn>
__device__ inline const u16* span_min_codes(ValueFn value, ValidFn valid, u32 nv, u32 k, const OwnerCodes& c, u16* a, u16* b, u32& p) {
    for (u32 t = threadIdx.x; t < nv; t += 256) a[t] = valid(t) ? owner_code(value(t), c) : (u16)0xFFFFu;
    __syncthreads();
    for (p = 1; 2 * p <= k; p *= 2) {
        for (u32 t = threadIdx.x; t < nv; t += 256) { const u16 x = a[t], y = t + p < nv ? a[t + p] : (u16)0xFFFFu; b[t] = x < y ? x : y; }
        __syncthreads();
        u16* const sw = a; a = b; b = sw;
    }
    return a;
}

// find-or-claim for a whole wave: every lane calls it together, act = the lane has a window (its k values at w, window start = store index i, position li in a
// list that is in window order where consecutive entries are consecutive windows of a read).  claimed: the lane created the key; found: it met its key in slot s.
// The walk of upsert_slot is cut in two.  (1) Every lane walks to the first slot that is empty (claims it) or carries its fingerprint.  (2) The fingerprint
// hits are confirmed: with all lanes' first stage behind them, the loads of the representatives are issued side by side instead of each at the end of its
// lane's own chain of probes — 0.713 -> 0.665 ms per 6.6 M windows, 36.6 -> 33.5 ms for the human data set (profiles/r05_x_insert_two_stage.txt).
// A lane whose hit CONTINUES its left neighbour's — the neighbour (window i - 1) sits in a slot whose representative is store index r, this lane's slot names
// r + 1 (r - 1 when the orientations cross), same orientation relation — is a LINK: k - 1 of its k comparisons are the neighbour's, it compares its newest
// value only (8 bytes instead of 8 k in three cache lines); it is confirmed when it and every lane between it and its HEAD (the nearest lane below that is not a
// link; lane 0 always is one, nothing crosses a wave) passed.  Nothing is taken on trust: every accepted match is a full comparison or follows from one.  Links
// need the neighbouring keys to have been created by neighbouring windows of ONE earlier read: common when a batch holds a copy or two of a region (a file
// streamed in 256-Mbase batches), rare when one launch inserts dozens of copies that race for the claim (the benchmark's 50x batches: no gain there; an
// experiment that compared 16 bytes of every representative — not exact, never shipped: profiles/r05_x_shortcmp.txt — bounds what links can give at -18 % / -22 %).
// A lane that fails either way walks on with full comparisons like upsert_slot.
__device__ inline u64 upsert_wave_h(const TableArgs& T, bool act, u32 li, u64 i, const u64* w, u32 k, bool rev, u64 h, bool& claimed, bool& found);
__device__ inline u64 upsert_wave(const TableArgs& T, bool act, u32 li, u64 i, const u64* w, u32 k, bool& claimed, bool& found) {
    bool rev = false; u64 h = 0;
    if (act) { rev = window_reversed(w, k); h = key_hash_window(w, k, rev); }
    return upsert_wave_h(T, act, li, i, w, k, rev, h, claimed, found);
}
// (rev, h: the window's orientation and key hash, computed by the caller)
__device__ inline u64 upsert_wave_h(const TableArgs& T, bool act, u32 li, u64 i, const u64* w, u32 k, bool rev, u64 h, bool& claimed, bool& found) {
    const int lane = threadIdx.x & 63;
    const u64 fp = (h >> 34) & T.fp_mask;
    const u64 myword_lo = ((u64)rev << 32) | (u64)(u32)i;
    auto eq = [&](u64 word) { return same_key_window(T.ks, word, w, rev); };
    // (1) to the first slot that is empty or carries the fingerprint
    u64 s = act ? home_slot(h, T.cap) : 0, word = EMPTY, probes = 0;
    claimed = false;
    bool cand = false;
    if (act) {
        for (; probes <= T.cap; ++probes) {
            u64 wv = load_relaxed(&T.tab[s].word);
            if (wv == EMPTY) {
                const u64 old = atomicCAS((unsigned long long*)&T.tab[s].word, (unsigned long long)EMPTY, (unsigned long long)((fp << 34) | myword_lo));
                if (old == EMPTY) { wave_agg_inc(T.n_distinct); claimed = true; break; }
                wv = old;
            }
            if ((wv >> 34) == fp) { word = wv; cand = true; break; }
            s = s + 1 == T.cap ? 0 : s + 1;
        }
        if (!claimed && !cand) { *T.probe_err = 1; s = ~0ull; }      // table full: cannot happen when it was sized from the true number of windows
    }
    // (2) heads and links
    const bool cross = rev != ((word & (1ull << 32)) != 0);
    const u32 rep = (u32)word;
    const u32 p_li = (u32)__shfl_up((int)li, 1, 64), p_rep = (u32)__shfl_up((int)rep, 1, 64);
    const int p_info = __shfl_up((int)((cand && !(word & (1ull << 33)) ? 1 : 0) | (cross ? 2 : 0)), 1, 64);
    const bool link = cand && !T.no_chain && lane > 0 && !(word & (1ull << 33)) && (p_info & 1) && p_li + 1 == li && ((p_info >> 1) & 1) == (int)cross &&
                      rep == (cross ? p_rep - 1u : p_rep + 1u);
    bool pass = false;
    if (cand) pass = link ? T.ks.mh[(u64)rep + (cross ? 0u : k - 1u)] == w[k - 1] : eq(word);
    const u64 heads = __ballot(!link), fails = __ballot(cand && !pass);
    found = pass;
    if (link && pass) {
        const int hp = 63 - __clzll((unsigned long long)(heads & ((2ull << lane) - 1ull)));      // the nearest head below: lane 0 is one
        found = ((fails >> hp) & ((2ull << (lane - hp)) - 1ull)) == 0;
    }
    if (T.link_ctr) { const u64 lm = __ballot(link && found); if (lane == 0 && lm) atomicAdd(T.link_ctr, (unsigned long long)__popcll(lm)); }
    if (cand && !found) {
        // another key behind this fingerprint, or a chain that broke in front of this lane: the plain walk, entered at this slot (a head has compared it already)
        const bool skip = !link;
        s = upsert_slot_from(T, h, myword_lo, eq, claimed, skip ? (s + 1 == T.cap ? 0 : s + 1) : s, probes + (skip ? 1 : 0));
        found = !claimed && s != ~0ull;
    }
    return s;
}

// Windows of the minimizers [i0, i1) of a batch -> counting table.  src/main.rs:756 — only reads with MORE than k minimizers contribute,
// so most minimizer indices start no window (15 kb reads at d = 0.002: 14 of 48), and with a partitioned table (replicated-sketch mode)
// most windows belong to other ranks.  One workgroup stages the OWN_SPAN + k - 1 hashes its span covers in LDS (coalesced), lists the
// local indices of the windows this rank has to insert, and then works the list off densely, so the long find-or-claim chains run on
// full wavefronts (0.80 -> 0.64 ms per 6.6 M windows against one thread per minimizer index).  Orientation, hash and the own side of the
// key comparison read the staged values.
constexpr int OWN_SPAN = 2048;
// the kernel's dynamic LDS, in the order it is carved up below; codes: partitioned table, the owner codes of the staged hashes
static size_t insert_windows_lds(const TableArgs& T) {
    const size_t codes = T.own_world > 1 && T.own_thr ? 2 * ((size_t)OWN_SPAN + T.ks.k) * sizeof(u16) : 0;
    return (OWN_SPAN + T.ks.k) * sizeof(u64) + OWN_SPAN * sizeof(u16) + 16 + OWN_SPAN + codes;
}
// GATED (the counting pre-filter, prefilter.hip): a window is inserted only when its admission bit is set — bit (i - adm_i0) of adm[], written by prefilter_admit_kernel
// for the batch that starts at adm_i0.  That is the only difference: the ungated instantiation is the kernel as it was (adm is never read; its instruction stream is
// the one of the kernel before the template, profiles/prefilter_notes.md), and both write every claim byte of their span.
template <bool GATED>
__global__ __launch_bounds__(256) void insert_windows_kernel(TableArgs T, const u64* __restrict__ mh, const u32* __restrict__ mread,
                                                                   const u64* __restrict__ roff, u64 i0, u64 i1, u32 slot0, u64 first_ordinal,
                                                                   u32* __restrict__ cap_err, const u64* __restrict__ i1_dev, u64 n_lim, const u64* __restrict__ adm, u64 adm_i0) {
    extern __shared__ u64 sh_keys[];           // [OWN_SPAN + k] keys, then u16 list[OWN_SPAN], then the counter, then u8 cl[OWN_SPAN], then (partitioned table) 2 x u16 codes[OWN_SPAN + k]
    if (cap_err[1]) return;
    // i1_dev: launched behind the sketch of the same batch before the host knew how many minimizers it has (i1 = an upper bound the grid was
    // sized for): the count comes from the device, workgroups behind it have nothing to do
    if (i1_dev) { i1 = *i1_dev; if (i0 + (u64)blockIdx.x * OWN_SPAN >= i1) return; }
    const u32 k = T.ks.k;
    u16* const list = (u16*)(sh_keys + OWN_SPAN + k);
    u32* const n_own = (u32*)(list + OWN_SPAN);
    u8* const cl = (u8*)(n_own + 4);             // [OWN_SPAN] claim bytes of the span (T.claim)
    const u64 b0 = i0 + (u64)blockIdx.x * OWN_SPAN;
    const u64 lim = b0 + OWN_SPAN + k - 1 < i1 ? b0 + OWN_SPAN + k - 1 : i1;
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    if (threadIdx.x == 0) *n_own = 0;
    if (T.claim) for (int u = threadIdx.x; u < OWN_SPAN / 8; u += 256) ((u64*)cl)[u] = 0;
    __syncthreads();
    // partitioned table: whose window is it?  From the codes of the staged hashes (see "owner codes"), or — no owner parameters — from the k values themselves
    const bool by_codes = T.own_world > 1 && T.own_thr != nullptr;
    const u16* mc = nullptr; u32 pc = 1; OwnerCodes oc{};
    if (by_codes) {
        u16* const ca = (u16*)(cl + OWN_SPAN);
        oc = owner_codes_of(OwnerSpec{T.own_world, T.own_thr});
        const u32 n_st = (u32)(lim - b0);
        mc = span_min_codes([&](u32 t) { return sh_keys[t]; }, [&](u32 t) { return t < n_st; }, OWN_SPAN + k - 1, k, oc, ca, ca + (OWN_SPAN + k), pc);
    }
#pragma unroll
    for (int u = 0; u < OWN_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        const u64 i = b0 + li;
        bool mine = false;
        bool own = i + k <= i1;
        if (GATED) { if (own) own = (adm[(i - adm_i0) >> 6] >> ((i - adm_i0) & 63)) & 1ull; }
        if (own && T.own_world > 1) {
            if (by_codes) { const u16 x = mc[li], y = mc[li + k - pc]; own = owner_of_code(x < y ? x : y, oc) == T.own_rank; }
            else own = window_owner(sh_keys + li, k, OwnerSpec{T.own_world, T.own_thr}) == T.own_rank;
        }
        if (own) {                                                        // ownership first: it needs no further loads
            const u32 slot = mread[i];
            const u64 rs = roff[slot], re = roff[slot + 1];
            mine = re - rs > k && i + k <= re;
        }
        const u64 m = __ballot(mine);
        u32 base = 0;
        if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(n_own, (u32)__popcll(m));
        base = __shfl(base, 0, 64);
        if (mine) list[base + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1))] = (u16)li;
    }
    __syncthreads();
    const u32 n = *n_own;
    if (threadIdx.x == 0 && n && T.own_world > 1) atomicAdd((unsigned long long*)ctr_shard(T.own_inserted), (unsigned long long)n);      // (checked against the senders' counts: partitioned tables only)
    for (u32 j0 = 0; j0 < n; j0 += 256) {          // (the same trip count for every lane: upsert_wave is a wave-wide call)
        const u32 j = j0 + threadIdx.x;
        bool act = j < n;
        const u32 li = act ? list[j] : 0u;
        const u64 i = b0 + li;
        u64 ord = 0;
        if (act) {
            const u32 slot = mread[i];
            const u64 win = i - roff[slot];
            if (win > WIN_MASK) { *cap_err = 1; act = false; }
            ord = ((first_ordinal + (slot - slot0)) << WIN_BITS) | win;
        }
        bool claimed, found;
        const u64 s = upsert_wave(T, act, li, i, sh_keys + li, k, claimed, found);
        if (claimed && T.claim) cl[li] = 1;
        if (found) record_hit(T, s, ord);
    }
    if (T.claim) {                             // the span's claim bytes, 64 consecutive bytes per wave and store (a slice's last workgroup stops at its end: n_lim)
        __syncthreads();
        const u64 hi = i1 - b0 < (u64)OWN_SPAN ? i1 - b0 : (u64)OWN_SPAN;
        for (u32 li = threadIdx.x; li < hi && li < n_lim - (u64)blockIdx.x * OWN_SPAN; li += 256) T.claim[b0 + li] = cl[li];
    }
}
// adm (null: every window): the admission bits of the batch that starts at minimizer index adm_i0, see insert_windows_kernel
void launch_insert_windows(const TableArgs& T, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 slot0,
                           u64 first_ordinal, u64* n_windows, u32* cap_err, hipStream_t s, const u64* i1_dev = nullptr, u64 n_starts = 0,
                           const u64* adm = nullptr, u64 adm_i0 = 0) {
    if (i1 <= i0) return;
    (void)n_windows;
    const u64 n = n_starts ? n_starts : i1 - i0;          // n_starts: only the window starts [i0, i0 + n_starts) (a slice; i1 stays the end of the batch)
    const dim3 grid((unsigned)((n + OWN_SPAN - 1) / OWN_SPAN));
    if (adm) hipLaunchKernelGGL(insert_windows_kernel<true>, grid, dim3(256), insert_windows_lds(T), s, T, mh, mread, roff, i0, i1, slot0, first_ordinal, cap_err, i1_dev, n, adm, adm_i0);
    else hipLaunchKernelGGL(insert_windows_kernel<false>, grid, dim3(256), insert_windows_lds(T), s, T, mh, mread, roff, i0, i1, slot0, first_ordinal, cap_err, i1_dev, n, adm, adm_i0);
}

// routed records (k canonical u64, ordinal, key hash) sitting in the arena at record index r0..
__global__ __launch_bounds__(256) void insert_records_kernel(TableArgs T, u64 r0, u64 r1, u64* __restrict__ n_windows) {
    const u64 r = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= r1) return;
    const u32 k = T.ks.k;
    const u64* key = T.ks.arena + r * (k + 2);
    const u64 h = key[k + 1];                  // computed by the sender (route_count_kernel)
    bool claimed;
    const u64 s = upsert_slot(T, h, (1ull << 33) | (u64)(u32)r, [&](u64 word) { return same_key_window(T.ks, word, key, false); }, claimed);   // record keys are canonical
    if (claimed || s == ~0ull) return;
    record_hit(T, s, key[k]);
    (void)n_windows;
}
void launch_insert_records(const TableArgs& T, u64 r0, u64 r1, u64* n_windows, hipStream_t s) {
    if (r1 <= r0) return;
    hipLaunchKernelGGL(insert_records_kernel, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, s, T, r0, r1, n_windows);
}

// z: small regions zeroed by the same launch (mdbg_reset: the shards of the key counter and three scalars — a launch of their own until round 6)
__global__ void clear_table_kernel(Slot* __restrict__ tab, u64 cap, u64* __restrict__ mx, u64 n_mx, ZeroList z) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    {
        const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
        for (int r = 0; r < 6; ++r) for (u64 i = i0; i < z.n[r]; i += stride) z.p[r][i] = 0;
        if (i0 == 0 && z.set_p) *z.set_p = z.set_v;
    }
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        uint4* p = (uint4*)(tab + i);
        p[0] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);     // word, m1
        p[1] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);                         // m2, count, pad
    }
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_mx; i += stride) mx[i] = EMPTY;
}
void launch_clear_table(Slot* tab, u64 cap, u64* mx, u64 n_mx, hipStream_t s, const ZeroList* z = nullptr) {
    ZeroList none{};
    hipLaunchKernelGGL(clear_table_kernel, dim3(2048), dim3(256), 0, s, tab, cap, mx, n_mx, z ? *z : none);
}

// grow: move every occupied slot of the old table into the new one (keys are unique: claim the first empty slot)
__global__ void rehash_kernel(const Slot* __restrict__ old, u64 old_cap, const u64* __restrict__ old_mx, TableArgs T) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_cap) return;
    const Slot e = old[i];
    if (e.word == EMPTY) return;
    const u64 h = key_hash_fn([&](u32 j) { return rep_elem(T.ks, e.word, j); }, T.ks.k);
    u64 s = home_slot(h, T.cap);
    for (;;) {
        const u64 oldw = atomicCAS((unsigned long long*)&T.tab[s].word, (unsigned long long)EMPTY, (unsigned long long)e.word);
        if (oldw == EMPTY) break;
        s = s + 1 == T.cap ? 0 : s + 1;
    }
    T.tab[s].m1 = e.m1; T.tab[s].m2 = e.m2; T.tab[s].count = e.count;
    for (u32 j = 0; j + 2 < T.A; ++j) T.mx[s * (T.A - 2) + j] = old_mx[i * (T.A - 2) + j];
}
void launch_rehash(const Slot* old, u64 old_cap, const u64* old_mx, const TableArgs& T, hipStream_t s) {
    hipLaunchKernelGGL(rehash_kernel, dim3((unsigned)((old_cap + 255) / 256)), dim3(256), 0, s, old, old_cap, old_mx, T);
}

// Device-side twin of table_reserve(): flags the batch when the table is too small for it, so that the host can launch
// the insert speculatively and needs one round trip per batch instead of two.  Same rule as slots_for() in api.inc.
// The number of keys in the table is summed from its shards here (one launch less in front of every insertion).
// carry / over_max (null: not used): the insertion was launched behind the batch's own sketch, before the host looked at it — when the sketch has to
// be repeated (a slab or the store was too small, or the 2^32 limit) the insertion must not happen either.
__global__ __launch_bounds__(256) void reserve_check_kernel(const u64* __restrict__ distinct_shards, u64* __restrict__ n_distinct, const u64* __restrict__ batch_windows, u64 cap,
                                                            u32* __restrict__ too_small, const u64* __restrict__ carry, u64 store_cap, const u32* __restrict__ over_max) {
    __shared__ u64 ws[4];
    u64 v = 0;
    for (int i = threadIdx.x; i < CTR_SHARDS; i += 256) v += distinct_shards[i];
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 nd = ws[0] + ws[1] + ws[2] + ws[3];
        *n_distinct = nd;
        const u64 n = nd + *batch_windows;
        bool skip = n + n / 2 + 1024 > cap;
        if (carry) skip = skip || *carry > store_cap || *carry >= 0xFFFFFFF0ull || (over_max && *over_max);
        *too_small = skip ? 1u : 0u;
    }
}
void launch_reserve_check(const u64* distinct_shards, u64* n_distinct, const u64* batch_windows, u64 cap, u32* too_small, hipStream_t s,
                          const u64* carry = nullptr, u64 store_cap = 0, const u32* over_max = nullptr) {
    hipLaunchKernelGGL(reserve_check_kernel, dim3(1), dim3(256), 0, s, distinct_shards, n_distinct, batch_windows, cap, too_small, carry, store_cap, over_max);
}

// count_windows_kernel + reserve_check_kernel in ONE launch (the insertion launched behind the batch's own sketch: two 8-microsecond kernels in a row in front of every
// insertion).  Every workgroup adds its reads' windows to *batch_windows and then to *done; the workgroup that brings *done to the grid size runs the check (the
// others' additions are visible to it: device-scope atomics, a fence on both sides) and sets *done back to zero for the next launch.
__global__ __launch_bounds__(1024) void count_reserve_kernel(const u64* __restrict__ roff, u32 slot0, u32 n_reads, u32 k, u64* __restrict__ batch_windows, u32* __restrict__ done,
                                                             const u64* __restrict__ distinct_shards, u64* __restrict__ n_distinct, u64 cap, u32* __restrict__ too_small,
                                                             const u64* __restrict__ carry, u64 store_cap, const u32* __restrict__ over_max) {
    __shared__ u64 ws[16];
    __shared__ u32 last;
    u64 w = 0;
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) { const u64 n = roff[slot0 + r + 1] - roff[slot0 + r]; if (n > k) w += n - k + 1; }
    for (int d = 32; d; d >>= 1) w += __shfl_down(w, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (int i = 0; i < 16; ++i) t += ws[i];
        if (t) atomicAdd((unsigned long long*)batch_windows, (unsigned long long)t);      // (at most 64 workgroups: two same-address atomics each, ~12 ns apiece)
        __threadfence();
        last = atomicAdd(done, 1u) + 1u == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    u64 v = 0;
    for (int i = threadIdx.x; i < CTR_SHARDS; i += 1024) v += distinct_shards[i];
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();                                   // (ws is read above by thread 0 only, long ago; the barrier is for its reuse)
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 nd = 0;
        for (int i = 0; i < 16; ++i) nd += ws[i];
        *n_distinct = nd;
        const u64 bw = __hip_atomic_load(batch_windows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 n = nd + bw;
        bool skip = n + n / 2 + 1024 > cap;                                                      // slots_for(), api.inc
        if (carry) skip = skip || *carry > store_cap || *carry >= 0xFFFFFFF0ull || (over_max && *over_max);
        *too_small = skip ? 1u : 0u;
        *done = 0;
    }
}
void launch_count_reserve(const u64* roff, u32 slot0, u32 n_reads, u32 k, u64* batch_windows, u32* done, const u64* distinct_shards, u64* n_distinct, u64 cap, u32* too_small,
                          const u64* carry, u64 store_cap, const u32* over_max, hipStream_t s) {
    hipLaunchKernelGGL(count_reserve_kernel, dim3(n_reads ? std::min<u32>(64u, (n_reads + 1023) / 1024) : 1), dim3(1024), 0, s, roff, slot0, n_reads, k, batch_windows, done, distinct_shards, n_distinct, cap,
                       too_small, carry, store_cap, over_max);
}

// A batch inserted in SLICES (dense settings: hundreds of millions of windows of which few are new keys — sizing the table for all of them would make it
// tens of GB): before slice `id` the table must have room for `bound` more keys (one per window start of the slice at most).  The first slice that does
// not fit sets *too_small (which makes it and every later insert kernel of the round return at once) and leaves its id; the host grows the table and
// resumes there.
__global__ __launch_bounds__(256) void slice_check_kernel(const u64* __restrict__ distinct_shards, u64* __restrict__ n_distinct, u64 bound, u64 cap, u32* __restrict__ too_small,
                                                          u64* __restrict__ fail_at, u64 id) {
    __shared__ u64 ws[4];
    if (*too_small) return;
    u64 v = 0;
    for (int i = threadIdx.x; i < CTR_SHARDS; i += 256) v += distinct_shards[i];
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 nd = ws[0] + ws[1] + ws[2] + ws[3];
        *n_distinct = nd;
        const u64 n = nd + bound;
        if (n + n / 2 + 1024 > cap) { *fail_at = id; *too_small = 1u; }
    }
}
void launch_slice_check(const u64* distinct_shards, u64* n_distinct, u64 bound, u64 cap, u32* too_small, u64* fail_at, u64 id, hipStream_t s) {
    hipLaunchKernelGGL(slice_check_kernel, dim3(1), dim3(256), 0, s, distinct_shards, n_distinct, bound, cap, too_small, fail_at, id);
}

// number of k-min-mer occurrences of a batch: sum over its reads of (n > k ? n - k + 1 : 0)   (src/main.rs:756-759)
__global__ __launch_bounds__(1024) void count_windows_kernel(const u64* __restrict__ roff, u32 slot0, u32 n_reads, u32 k, u64* __restrict__ out) {
    __shared__ u64 ws[16];
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u64 w = 0;
    if (r < n_reads) { const u64 n = roff[slot0 + r + 1] - roff[slot0 + r]; if (n > k) w = n - k + 1; }
    for (int d = 32; d; d >>= 1) w += __shfl_down(w, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {                  // one atomic per workgroup: same-address atomics serialise (~12 ns each)
        u64 t = 0;
        for (int i = 0; i < 16; ++i) t += ws[i];
        if (t) atomicAdd((unsigned long long*)out, (unsigned long long)t);
    }
}
void launch_count_windows(const u64* roff, u32 slot0, u32 n_reads, u32 k, u64* out, hipStream_t s) {
    if (!n_reads) return;
    hipLaunchKernelGGL(count_windows_kernel, dim3((n_reads + 1023) / 1024), dim3(1024), 0, s, roff, slot0, n_reads, k, out);
}

// lookup without insertion: slot of a key that is known to be in the table, or ~0 (keys of other ranks)
template <class EqFn>
__device__ inline u64 find_slot(const TableArgs& T, u64 h, EqFn same_key) {
    const u64 fp = (h >> 34) & T.fp_mask;
    u64 s = home_slot(h, T.cap);
    for (;;) {
        const u64 w = load_relaxed(&T.tab[s].word);
        if (w == EMPTY) return ~0ull;
        if ((w >> 34) == fp && same_key(w)) return s;
        s = s + 1 == T.cap ? 0 : s + 1;
    }
}
// --read_stats (src/main.rs:939-1004): abundance of the k-min-mer that starts at minimizer i in the FILTERED table, 0 when it
// is absent or below the abundance filter; NO_WINDOW where no window starts (fewer than k minimizers left in the read, or
// a read with at most k minimizers: src/main.rs:950, strictly more than k).
constexpr u32 NO_WINDOW = 0xFFFFFFFFu;
static size_t query_windows_lds(const TableArgs& T) { return (256 + T.ks.k) * 8; }      // the 256 + k - 1 hashes a workgroup's windows cover (+ one)
__global__ __launch_bounds__(256) void query_windows_kernel(TableArgs T, u32 A_filter, const u64* __restrict__ mh, const u32* __restrict__ mread,
                                                            const u64* __restrict__ roff, u64 i0, u64 i1, u32* __restrict__ out) {
    extern __shared__ u64 sh_keys[];
    const u32 k = T.ks.k;
    const u64 b0 = i0 + (u64)blockIdx.x * 256;
    const u64 lim = b0 + 256 + k - 1 < i1 ? b0 + 256 + k - 1 : i1;
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    const u64 i = b0 + threadIdx.x;
    bool active = i < i1;
    if (active) {
        const u32 slot = mread[i];
        const u64 rs = roff[slot], re = roff[slot + 1];
        active = re - rs > k && i + k <= re;
        if (!active) out[i - i0] = NO_WINDOW;
    }
    __syncthreads();
    if (!active) return;
    const u64* w = sh_keys + threadIdx.x;
    const bool rev = window_reversed(w, k);
    u32 ab = 0;
    if (T.cap) {
        const u64 s = find_slot(T, key_hash_window(w, k, rev), [&](u64 word) { return same_key_window(T.ks, word, w, rev); });
        if (s != ~0ull) {
            const u32 count = T.tab[s].count + 1u;
            if (A_filter == 1 || (u16)count >= (u16)A_filter) ab = (u16)count;      // dbg_nodes.retain (main.rs:927), u16 abundance
        }
    }
    out[i - i0] = ab;
}
void launch_query_windows(const TableArgs& T, u32 A_filter, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32* out, hipStream_t s) {
    if (i1 <= i0) return;
    const u64 n = i1 - i0;
    hipLaunchKernelGGL(query_windows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), query_windows_lds(T), s, T, A_filter, mh, mread, roff, i0, i1, out);
}
