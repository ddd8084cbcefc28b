// owner.hip — the multi-GPU partition of the key space, replicated-sketch mode (gfx950): the thresholds of the owner function, the counts of a rank's windows,
// the owner lists a sketching rank makes for its peers, the segments of hashes that travel with them, and the insertion of listed windows.
// The owner function itself (OwnerSpec, window_owner, owner_of_min) and the owner codes stand in table.hip, in front of insert_windows_kernel, which needs them.
#include "mdbg_dev.h"
// thr[r - 1] = bound * (1 - (1 - r / world)^(1 / k)), r = 1 .. world - 1: the values at which the distribution function of the window minimum,
// 1 - (1 - v / bound)^k, passes r / world.  Computed ONCE per (k, world, bound) on the device (every rank runs the same code on the same
// hardware: identical thresholds without any host floating point), the windows are then placed by integer comparisons.
__global__ void owner_thresholds_kernel(double bound, u32 k, u32 world, u64* __restrict__ thr) {
    const u32 r = threadIdx.x + 1;
    if (threadIdx.x == 0) thr[0] = 0;               // no measured table (yet)
    thr += OWNER_THR_AT;
    if (r >= world) return;
    const double x = -expm1(log1p(-(double)r / (double)world) / (double)k);
    double v = x * bound;
    thr[r - 1] = v >= 18446744073709549568.0 ? ~0ull : (u64)v;
}
void launch_owner_thresholds(double bound, u32 k, u32 world, u64* thr, hipStream_t s) {
    if (world > 1) hipLaunchKernelGGL(owner_thresholds_kernel, dim3(1), dim3(64), 0, s, bound, k, world, thr);
}

// the same, counting only the windows owned by `rank` (replicated-sketch mode); one thread per minimizer index
__global__ __launch_bounds__(256) void count_owned_windows_kernel(const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i0, u64 i1,
                                                                  u32 k, u32 world, const u64* thr, u32 rank, u64* __restrict__ out) {
    constexpr int WPT = 4;                   // four candidates per thread: their dependent loads overlap
    const u64 b0 = i0 + (u64)blockIdx.x * (256 * WPT);
    u32 slot[WPT]; bool ok[WPT];
#pragma unroll
    for (int u = 0; u < WPT; ++u) { const u64 i = b0 + u * 256 + threadIdx.x; ok[u] = i < i1; slot[u] = ok[u] ? mread[i] : 0; }
    u32 mine = 0;
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
        const u64 i = b0 + u * 256 + threadIdx.x;
        if (ok[u]) {
            const u64 rs = roff[slot[u]], re = roff[slot[u] + 1];
            if (re - rs > k && i + k <= re && window_owner(mh + i, k, OwnerSpec{world, thr}) == rank) ++mine;
        }
    }
    for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd((unsigned long long*)ctr_shard(out), (unsigned long long)mine);
}
void launch_count_owned_windows(const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u32 world, const u64* thr, u32 rank, u64* out_shards, hipStream_t s) {
    if (i1 > i0) hipLaunchKernelGGL(count_owned_windows_kernel, dim3((unsigned)((i1 - i0 + 1023) / 1024)), dim3(256), 0, s, mh, mread, roff, i0, i1, k, world, thr, rank, out_shards);
}
// per-owner window counts of a batch (what a rank tells its peers, so that nobody has to re-count a foreign sketch)
static size_t owner_hist_lds(u32 world) { return world * sizeof(u32); }      // hist[world]
__global__ __launch_bounds__(256) void owner_hist_kernel(const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i0, u64 i1,
                                                         u32 k, u32 world, const u64* thr, u64* __restrict__ counts) {
    extern __shared__ u32 hist[];
    for (u32 t = threadIdx.x; t < world; t += 256) hist[t] = 0;
    __syncthreads();
    constexpr int WPT = 4;
    const u64 b0 = i0 + (u64)blockIdx.x * (256 * WPT);
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
        const u64 i = b0 + u * 256 + threadIdx.x;
        if (i < i1) {
            const u32 slot = mread[i];
            const u64 rs = roff[slot], re = roff[slot + 1];
            if (re - rs > k && i + k <= re) atomicAdd(&hist[window_owner(mh + i, k, OwnerSpec{world, thr})], 1u);
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < world; t += 256) if (hist[t]) atomicAdd((unsigned long long*)&counts[t], (unsigned long long)hist[t]);
}
void launch_owner_hist(const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u32 world, const u64* thr, u64* counts, hipStream_t s) {
    if (i1 > i0) hipLaunchKernelGGL(owner_hist_kernel, dim3((unsigned)((i1 - i0 + 1023) / 1024)), dim3(256), owner_hist_lds(world), s, mh, mread, roff, i0, i1, k, world, thr, counts);
}

// ---- owner lists (replicated-sketch mode) -----------------------------------------------------------------------------------------
// The rank that sketched a batch also lists, per owning rank, the windows that rank owns (u32 index of the window's first minimizer,
// relative to the batch, and the index of its read in the batch: a pair of u32): 8 bytes per window shipped with the sketch, so that a
// receiver inserts exactly its windows instead of scanning every foreign sketch for them, and needs no minimizer -> read map of the
// foreign sketch either — the per-rank work no longer grows with the number of ranks.
// Two passes with per-block counts and a scan in between (deterministic bucket sizes, no same-address atomics on global counters).
constexpr int OWNL_SPAN = 2048;               // window starts per block: the span of hashes a receiving workgroup stages in LDS (16 KB + k values)
constexpr u32 OWNL_MAX_WORLD = 64;
struct OwnerBases { u64 b[OWNL_MAX_WORLD]; }; // start of every owner's bucket in the list
__device__ inline bool window_starts_at(const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i, u64 i1, u32 k) {
    if (i >= i1) return false;
    const u32 slot = mread[i];
    const u64 rs = roff[slot], re = roff[slot + 1];
    return re - rs > k && i + k <= re;
}
// The count pass also leaves every window start's owner in owner_of[] (0xFF: no window starts there) for the write pass.  The smallest hash
// of all the span's windows comes from LDS: the span's hashes are staged once and reduced by doubling (min over 2, 4, ... p <= k values; a
// window of k is two overlapping stretches of p) — read from HBM window by window it was 35 loads each, 1.4 ms per 6.6 M windows.
constexpr u32 OWNL_LDS_MAX_K = 1024;          // longer k: the plain loop (2 x (OWNL_SPAN + k) values have to fit the default 64 KB of dynamic LDS)
// dynamic LDS of the kernels that reduce a span's owner codes by doubling (span_min_codes): two arrays of u16, none for the plain loop of a longer k
static size_t owner_span_codes_lds(u32 k) { return k <= OWNL_LDS_MAX_K ? 2 * ((size_t)OWNL_SPAN + k) * sizeof(u16) : 0; }
// window minima of a batch counted per bin of the value range (hist[OWNER_BINS], added to): what the measured owner table is made from
__global__ __launch_bounds__(256) void owner_bins_kernel(const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i0, u64 i1, u32 k, u64 mul,
                                                         unsigned long long* __restrict__ hist) {
    extern __shared__ u64 sh_min[];                   // k <= OWNL_LDS_MAX_K: two arrays of OWNL_SPAN + k - 1 codes (u16)
    const u64 b0 = i0 + (u64)blockIdx.x * OWNL_SPAN;
    const bool staged = k <= OWNL_LDS_MAX_K;
    OwnerCodes oc{}; oc.mul = mul;                    // (bins: the codes are the bins themselves)
    const u16* cur = nullptr; u32 p = 1;
    if (staged) { u16* const ca = (u16*)sh_min; cur = span_min_codes([&](u32 t) { return mh[b0 + t]; }, [&](u32 t) { return b0 + t < i1; }, OWNL_SPAN + k - 1, k, oc, ca, ca + (OWNL_SPAN + k), p); }
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int u = 0; u < OWNL_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        const u64 i = b0 + li;
        u32 bin = 0xFFFFFFFFu;
        if (window_starts_at(mread, roff, i, i1, k)) {
            if (staged) { const u16 x = cur[li], y = cur[li + k - p]; bin = x < y ? x : y; }
            else { u64 m = mh[i]; for (u32 j = 1; j < k; ++j) { const u64 x = mh[i + j]; m = x < m ? x : m; } bin = owner_code(m, oc); }
        }
        // one atomic per distinct bin of the wave (the heavy bins are hit by several lanes of every wave)
        for (u64 todo = __ballot(bin != 0xFFFFFFFFu); todo;) {
            const u32 bb = (u32)__shfl((int)bin, __ffsll((unsigned long long)todo) - 1, 64);
            const u64 mm = __ballot(bin == bb);
            if (bin == bb && (mm & ((1ull << lane) - 1)) == 0) atomicAdd(&hist[bb], (unsigned long long)__popcll(mm));
            todo &= ~mm;
        }
    }
}
void launch_owner_bins(const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u64 mul, u64* hist, hipStream_t s) {
    if (i1 > i0) hipLaunchKernelGGL(owner_bins_kernel, dim3((unsigned)((i1 - i0 + OWNL_SPAN - 1) / OWNL_SPAN)), dim3(256), owner_span_codes_lds(k), s, mh, mread, roff, i0, i1, k, mul, (unsigned long long*)hist);
}
__global__ __launch_bounds__(256) void owner_list_count_kernel(const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i0, u64 i1,
                                                               u32 k, u32 world, const u64* thr, u32* __restrict__ blk_cnt, u8* __restrict__ owner_of) {
    extern __shared__ u64 sh_min[];               // owner parameters and k <= OWNL_LDS_MAX_K: two arrays of OWNL_SPAN + k - 1 owner codes (u16), see "owner codes"
    __shared__ u32 hist[OWNL_MAX_WORLD];
    if (threadIdx.x < world) hist[threadIdx.x] = 0;
    const u64 b0 = i0 + (u64)blockIdx.x * OWNL_SPAN;
    const OwnerSpec os{world, thr};
    const bool staged = k <= OWNL_LDS_MAX_K && thr != nullptr && world > 1;
    OwnerCodes oc{}; const u16* cur = nullptr; u32 p = 1;
    if (staged) {
        // the hashes are turned into codes as they are read: nothing but 2 x 2 bytes per element is staged (round 3 - 5: the u64 values, 33 KB of LDS per workgroup)
        oc = owner_codes_of(os);
        u16* const ca = (u16*)sh_min;
        cur = span_min_codes([&](u32 t) { return mh[b0 + t]; }, [&](u32 t) { return b0 + t < i1; }, OWNL_SPAN + k - 1, k, oc, ca, ca + (OWNL_SPAN + k), p);
    } else __syncthreads();
#pragma unroll
    for (int u = 0; u < OWNL_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        const u64 i = b0 + li;
        u32 o = 0xFFu;
        if (window_starts_at(mread, roff, i, i1, k)) {
            if (staged) { const u16 x = cur[li], y = cur[li + k - p]; o = owner_of_code(x < y ? x : y, oc); }
            else o = window_owner(mh + i, k, os);
            atomicAdd(&hist[o], 1u);
        }
        if (i < i1) owner_of[i - i0] = (u8)o;
    }
    __syncthreads();
    if (threadIdx.x < world) blk_cnt[(size_t)blockIdx.x * world + threadIdx.x] = hist[threadIdx.x];
}
void launch_owner_list_count(const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u32 world, const u64* thr, u32* blk_cnt, u8* owner_of, hipStream_t s) {
    if (i1 > i0) hipLaunchKernelGGL(owner_list_count_kernel, dim3((unsigned)((i1 - i0 + OWNL_SPAN - 1) / OWNL_SPAN)), dim3(256), owner_span_codes_lds(k), s, mh, mread, roff, i0, i1, k, world, thr, blk_cnt, owner_of);
}
// Every owner's bucket comes out sorted by window start (the segments below are differences of neighbouring entries): the entries of a
// workgroup's span are ranked per owner in index order — lanes of a wave by ballots, the 32 (iteration, wave) groups by a prefix in LDS.
__global__ __launch_bounds__(256) void owner_list_write_kernel(const u64* __restrict__ mh, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 i0, u64 i1,
                                                               u32 k, u32 world, const u64* thr, u32 slot0, const u64* __restrict__ blk_off, OwnerBases bases, u32* __restrict__ list,
                                                               const u8* __restrict__ owner_of, u32 direct_owner, u32* __restrict__ direct_dst) {
    // direct_owner (< world): that owner's bucket is not part of `list` (its bases entry is unused): it goes to direct_dst, the place the rank keeps its own
    // share of its own batch (api.inc, owner_lists_impl) — until round 5 the bucket was written to the list and copied there (368 MB per 19.5-Gbase batch at one rank) —,
    // or, direct_dst == null, NOWHERE: since round 6 the multi-GPU layer inserts a rank's own windows of its own batch with insert_windows_kernel, which finds them itself
    // (owner codes of the hashes it stages anyway), so that bucket is neither written nor read nor cut into spans
    constexpr int NG = OWNL_SPAN / 64;
    __shared__ u32 grp[NG][OWNL_MAX_WORLD];
    for (int t = threadIdx.x; t < NG * (int)OWNL_MAX_WORLD; t += 256) ((u32*)grp)[t] = 0;
    __syncthreads();
    const u64 b0 = i0 + (u64)blockIdx.x * OWNL_SPAN;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr u32 NONE = 0xFFFFFFFFu;
    u32 own[OWNL_SPAN / 256], rank[OWNL_SPAN / 256], slot_of[OWNL_SPAN / 256];
#pragma unroll
    for (int u = 0; u < OWNL_SPAN / 256; ++u) {
        const u64 i = b0 + u * 256 + threadIdx.x;
        u32 o = NONE, slot = 0;
        if (i < i1) { const u32 ob = owner_of[i - i0]; if (ob != 0xFFu) { o = ob; slot = mread[i]; } }      // (the count pass decided which starts are windows, and whose)
        u32 r = 0;
        for (u64 todo = __ballot(o != NONE); todo;) {
            const u32 oo = (u32)__shfl((int)o, __ffsll((unsigned long long)todo) - 1, 64);
            const u64 m = __ballot(o == oo);
            if (o == oo) { r = (u32)__popcll(m & ((1ull << lane) - 1)); if (r == 0) grp[u * 4 + wv][oo] = (u32)__popcll(m); }
            todo &= ~m;
        }
        own[u] = o; rank[u] = r; slot_of[u] = slot;
    }
    __syncthreads();
    if (threadIdx.x < world) { u32 run = 0; for (int g = 0; g < NG; ++g) { const u32 c = grp[g][threadIdx.x]; grp[g][threadIdx.x] = run; run += c; } }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < OWNL_SPAN / 256; ++u) {
        const u32 o = own[u];
        if (o == NONE || (o == direct_owner && !direct_dst)) continue;
        const u64 i = b0 + u * 256 + threadIdx.x;
        const u64 at = blk_off[(size_t)blockIdx.x * world + o] + grp[u * 4 + wv][o] + rank[u];
        uint2* const e = o == direct_owner ? (uint2*)direct_dst + at : (uint2*)list + (bases.b[o] + at);
        *e = make_uint2((u32)(i - i0), slot_of[u] - slot0);        // window start and its read, both relative to the batch
    }
}
void launch_owner_list_write(const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u32 world, const u64* thr, u32 slot0, const u64* blk_off, const OwnerBases& bases, u32* list, const u8* owner_of, hipStream_t s,
                             u32 direct_owner = 0xFFFFFFFFu, u32* direct_dst = nullptr) {
    if (i1 > i0) hipLaunchKernelGGL(owner_list_write_kernel, dim3((unsigned)((i1 - i0 + OWNL_SPAN - 1) / OWNL_SPAN)), dim3(256), 0, s, mh, mread, roff, i0, i1, k, world, thr, slot0, blk_off, bases, list, owner_of, direct_owner, direct_dst);
}

// ---- segments: the hashes a rank's listed windows need, without the rest of the sketch -----------------------------------------------------------
// A bucket of the owner lists is sorted by window start w; the union of the windows' [w, w + k) is shipped as, per entry, the hashes it adds
// to the entries in front of it: all k when the window in front (same bucket) starts k or more earlier, else the last (w - w_prev) ones.  Both
// sides derive the same counts and their prefix from the list alone, so nothing but the list and the packed hashes travels.
// buckets: [n_buckets + 1] first entries (ascending); src / dst: hash index of window start 0 of every bucket.
struct SegBuckets { u64 start[OWNL_MAX_WORLD + 1]; u64 base[OWNL_MAX_WORLD]; u64 lim[OWNL_MAX_WORLD]; u32 n; u32 skip; };      // lim: hashes of the bucket's sketch (a window past
                                                                                                                                // it is skipped); skip: a bucket that ships nothing (the sender's own), or ~0
__device__ inline u32 seg_bucket_of(const SegBuckets& B, u64 j) {
    u32 lo = 0, hi = B.n - 1;
    while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (B.start[mid] <= j) lo = mid; else hi = mid - 1; }
    return lo;
}
// hashes entry j adds (b: its bucket)
__device__ inline u32 seg_add_of(const uint2* __restrict__ list, u64 j, u32 k, const SegBuckets& B, u32& b) {
    b = seg_bucket_of(B, j);
    if (b == B.skip) return 0;
    if (j && B.start[b] != j) { const u32 d = list[j].x - list[j - 1].x; if (d < k) return d; }
    return k;
}
// The counts are never stored: a pass over the list sums them per SEG_BLOCK entries (tile_scan_top_kernel turns the sums into bases), the copy pass derives them again
// and scans them inside its workgroup.  (Rounds 3 - 5 wrote a u32 count and a u64 prefix per entry and read both back: 1.98 ms per side for the 46 M entries of a
// 19.5-Gbase batch at eight ranks, 1.20 with the copy kernel below alone, profiles/r06_rank_w8.txt.)
constexpr u32 SEG_BLOCK = 4096;          // list entries per workgroup of the segment passes (one base per block: the single-workgroup scan of the bases stays short)
__global__ __launch_bounds__(256) void seg_sums_kernel(const uint2* __restrict__ list, u64 n, u32 k, SegBuckets B, u64* __restrict__ block_sum) {
    __shared__ u32 ws[4];
    u32 v = 0;
#pragma unroll
    for (int q = 0; q < SEG_BLOCK / 256; ++q) { const u64 j = (u64)blockIdx.x * SEG_BLOCK + q * 256 + threadIdx.x; u32 b; if (j < n) v += seg_add_of(list, j, k, B, b); }
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) block_sum[blockIdx.x] = (u64)ws[0] + ws[1] + ws[2] + ws[3];
}
// out[b] = first payload index of bucket b, out[B.n] = total (one workgroup per value; block_base: the scanned sums, total: the scan's carry)
__global__ __launch_bounds__(256) void seg_pick_kernel(const uint2* __restrict__ list, u64 n, u32 k, SegBuckets B, const u64* __restrict__ block_base, const u64* __restrict__ total,
                                                       u64* __restrict__ out) {
    __shared__ u32 ws[4];
    const u32 bq = blockIdx.x;
    const u64 j1 = bq < B.n ? B.start[bq] : n;
    if (j1 >= n) { if (threadIdx.x == 0) out[bq] = total[0]; return; }
    const u64 j0 = j1 - j1 % SEG_BLOCK;
    u32 v = 0;
#pragma unroll
    for (int q = 0; q < SEG_BLOCK / 256; ++q) { const u64 j = j0 + q * 256 + threadIdx.x; u32 b; if (j < j1) v += seg_add_of(list, j, k, B, b); }
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[bq] = block_base[j0 / SEG_BLOCK] + ws[0] + ws[1] + ws[2] + ws[3];
}
// counts and prefix of the list's segments: scan_tmp[n / SEG_BLOCK + 2] <- payload index of every SEG_BLOCK-entry block's first entry, carry[0] (zero on entry) <- total,
// picks[B.n + 1] <- first payload index of every bucket and the total.  launch_seg_copy then packs / scatters with scan_tmp.
void launch_seg_prefix(const u32* list, u64 n, u32 k, const SegBuckets& B, u64* scan_tmp, u64* carry, u64* picks, hipStream_t s) {
    if (!n) return;
    const u32 nb = (u32)((n + SEG_BLOCK - 1) / SEG_BLOCK);
    hipLaunchKernelGGL(seg_sums_kernel, dim3(nb), dim3(256), 0, s, (const uint2*)list, n, k, B, scan_tmp);
    hipLaunchKernelGGL(tile_scan_top_kernel, dim3(1), dim3(256), 0, s, nb, scan_tmp, carry);
    hipLaunchKernelGGL(seg_pick_kernel, dim3(B.n + 1), dim3(256), 0, s, (const uint2*)list, n, k, B, scan_tmp, carry, picks);
}
// pack (to_store = 0): payload[prefix of j ..) <- the last (count of j) hashes of window j read from the store; scatter (to_store = 1): the other way.
// A workgroup takes SEG_BLOCK consecutive entries, 256 at a time: their parts of the payload are one contiguous stretch, which its threads walk element by element (the entry
// of an element: a search among the 256 prefixes in LDS) — every load and store of the payload side is coalesced, the store side runs along the windows' runs.  (Rounds
// 3 - 5: one thread per entry copying its values in a loop: a run's first window copies k values, the others one or two — every wave waited for its run heads, 8 bytes
// per lane and round trip.)
__global__ __launch_bounds__(256) void seg_copy_kernel(const uint2* __restrict__ list, u64 n, u32 k, SegBuckets B, const u64* __restrict__ block_base,
                                                       u64* __restrict__ store, u64* __restrict__ payload, u64 payload_n, u32 to_store) {
    __shared__ u32 lpre[256];
    __shared__ u64 laddr[256];
    __shared__ u32 tmp[8];
    u64 P0 = block_base[blockIdx.x];
#pragma unroll 1
    for (int q = 0; q < SEG_BLOCK / 256; ++q) {
        const u64 j = (u64)blockIdx.x * SEG_BLOCK + q * 256 + threadIdx.x;
        u32 a = 0, b = 0, x = 0;
        if (j < n) { a = seg_add_of(list, j, k, B, b); x = list[j].x; }
        u32 T;
        const u32 excl = block_excl_scan_256(a, tmp, T);          // (its barriers also keep this round's LDS writes behind the last round's reads)
        u64 at = ~0ull;
        if (j < n && !((u64)x + k > B.lim[b] || P0 + excl + a > payload_n)) at = B.base[b] + x + (k - a);      // (a wrong list: reported by the size check of the round / the count check of the insertion)
        lpre[threadIdx.x] = j < n ? excl : 0xFFFFFFFFu;
        laddr[threadIdx.x] = at;
        __syncthreads();
        for (u32 e = threadIdx.x; e < T; e += 256) {
            u32 lo = 0, hi = 255;                      // the last entry whose prefix is <= e (entries that add nothing share their prefix with the one behind them)
#pragma unroll
            for (int st = 0; st < 8; ++st) { const u32 mid = (lo + hi + 1) >> 1; if (lpre[mid] <= e) lo = mid; else hi = mid - 1; }
            const u64 src = laddr[lo];
            if (src == ~0ull) continue;
            u64* const h = store + src + (e - lpre[lo]);
            u64* const pp = payload + P0 + e;
            if (to_store) *h = *pp; else *pp = *h;
        }
        P0 += T;
    }
}
void launch_seg_copy(const u32* list, u64 n, u32 k, const SegBuckets& B, const u64* scan_tmp, u64* store, u64* payload, u64 payload_n, bool to_store, hipStream_t s) {
    if (n) hipLaunchKernelGGL(seg_copy_kernel, dim3((unsigned)((n + SEG_BLOCK - 1) / SEG_BLOCK)), dim3(256), 0, s, (const uint2*)list, n, k, B, scan_tmp, store, payload, payload_n, to_store ? 1u : 0u);
}

// ---- insertion of listed windows ------------------------------------------------------------------------------------------------------------------
__device__ inline bool listed_check(u64 j) { return (((u32)j * 0x9E3779B1u) >> 28) == 0; }      // one list entry in 16
// inserts exactly the listed windows of the batch whose minimizers start at m0 (keys are read from the resident store)
// multi (non-null): the lists of SEVERAL batches in one launch — entry j belongs to batch b with multi[b].start <= j < multi[b + 1].start (n_multi batches
// and a closing entry); the per-batch arguments then come from the table.  (At 8 ranks and two chunks per step a rank inserts from 16 listed batches:
// 16 launches of ~0.4 M windows each.)
struct ListedBatch { u64 start, m0, m1, first_ordinal; const u32* list; u32 slot0, n_reads; };
// The per-entry kernel.  Its predecessor (rounds 3 - 5) waited on chains of dependent loads: four values per round trip of its hash loop (nine round trips at k = 35), k more
// for the owner check that one lane in 16 made (and every wave has such a lane): ~90 us per workgroup at full occupancy, 5.4 M windows/ms on a rank of eight
// (profiles/r06_rank_w8_ab.txt) against 10.8 M for the local kernel, whose values lie in LDS.  Here a window is read ONCE, sixteen values per round trip: hash and smallest
// value together (so EVERY entry's owner is re-derived, not one in 16), the batch of a wave's entries is found once per wave, and the walk is upsert_wave's: a bucket of the
// owner lists is sorted by window start and a rank's windows come in runs, so neighbouring lanes hold neighbouring windows, confirm each other as links, and their loads fall
// into the same cache lines.  8.4 M windows/ms.
__global__ __launch_bounds__(256) void insert_listed_entries_kernel(TableArgs T, const u64* __restrict__ mh, u32* __restrict__ mread, const u64* __restrict__ roff,
                                                                    u64 m0, u64 m1, const u32* __restrict__ list, u64 n, u32 slot0, u32 n_reads, u64 first_ordinal,
                                                                    u32* __restrict__ cap_err, const ListedBatch* __restrict__ multi, u32 n_multi) {
    if (cap_err[1]) return;
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 k = T.ks.k;
    bool ok = j < n;
    u64 i = 0, rs = 0; u32 slot = 0;
    u64 jl = j;
    if (multi) {
        // the batch of the wave's FIRST entry, searched once per wave on scalar loads; a lane behind the next batch's start (a wave across a boundary) searches for itself
        const u64 jw0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
        u64 jw = ((u64)__builtin_amdgcn_readfirstlane((u32)(jw0 >> 32)) << 32) | (u64)__builtin_amdgcn_readfirstlane((u32)jw0);
        if (jw >= n) jw = n - 1;
        u32 lo = 0, hi = n_multi - 1;
        while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (multi[mid].start <= jw) lo = mid; else hi = mid - 1; }
        if (ok && multi[lo + 1].start <= j) {          // (multi[n_multi] is the closing entry: start = n)
            hi = n_multi - 1;
            while (lo < hi) { const u32 mid = (lo + hi + 1) >> 1; if (multi[mid].start <= j) lo = mid; else hi = mid - 1; }
        }
        const ListedBatch b = multi[lo];
        m0 = b.m0; m1 = b.m1; list = b.list; slot0 = b.slot0; n_reads = b.n_reads; first_ordinal = b.first_ordinal; jl = j - b.start;
    }
    if (ok) {
        const uint2 e = ((const uint2*)list)[jl];
        i = m0 + e.x; slot = slot0 + e.y; ok = e.y < n_reads && i + k <= m1;
    }
    const u64* const w = mh + i;
    bool rev = false; u64 h = 0;
    if (ok) {                                      // a wrong list is caught by the count check
        // one round trip: the read's offsets and the window's two ends (the orientation is decided by them unless they are equal)
        const u64 w_first = w[0], w_last = w[k - 1];
        rs = roff[slot]; const u64 re = roff[slot + 1];
        ok = i >= rs && re - rs > k && i + k <= re;
        if (ok) {
            rev = w_first != w_last ? w_first > w_last : window_reversed(w, k);
            u64 smallest;
            h = key_hash_window_hbm(w, k, rev, smallest);
            ok = owner_of_min(smallest, k, OwnerSpec{T.own_world, T.own_thr}) == T.own_rank;      // a sender that disagrees about the owner function: the count check fails
        }
    }
    wave_count_add(ok, T.own_inserted);
    const u64 win = i - rs;
    if (ok && win > WIN_MASK) { *cap_err = 1; ok = false; }
    const u64 ord = ((first_ordinal + (slot - slot0)) << WIN_BITS) | win;
    bool claimed, found;
    const u64 s = upsert_wave_h(T, ok, (u32)i, i, w, k, rev, h, claimed, found);      // (li = the store index: consecutive windows of a read are consecutive indices; no lane leaves early)
    if (claimed) { mread[i] = slot; if (T.claim) T.claim[i] = 1; }      // (the batch's bytes of the claim map were zeroed in front of the launch: api.inc, insert_resident_impl)
    if (found) record_hit(T, s, ord);
}
// (95 registers = five waves per SIMD; forced to six or eight — 12 / 84 bytes of scratch — the kernel is slower: 5.87 / 7.00 against 5.48 ms per 46 M windows)
static void launch_listed_entries(const TableArgs& T, const u64* mh, u32* mread, const u64* roff, u64 m0, u64 m1, const u32* list, u64 n, u32 slot0, u32 n_reads, u64 first_ordinal,
                                  u32* cap_err, const ListedBatch* multi, u32 n_multi, hipStream_t s) {
    hipLaunchKernelGGL(insert_listed_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, mh, mread, roff, m0, m1, list, n, slot0, n_reads, first_ordinal, cap_err, multi, n_multi);
}
// The lists are written span by span (owner_list_write_kernel: the entries of one OWNL_SPAN of window starts are contiguous, in any order
// inside it), so the receiver can work span-wise too: seg[q] = first list entry of span q or later (seg[] is pre-filled with n).
__global__ __launch_bounds__(256) void list_segments_kernel(const u32* __restrict__ list, u64 n, u32 n_spans, u32* __restrict__ seg) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 last = n_spans - 1;
    u32 b = list[2 * j] / OWNL_SPAN; if (b > last) b = last;                 // entries out of range are rejected by the insert kernel
    int pb = -1;
    if (j) { u32 q = list[2 * j - 2] / OWNL_SPAN; if (q > last) q = last; pb = (int)q; }
    for (int q = pb + 1; q <= (int)b; ++q) seg[q] = (u32)j;                 // all spans' loops together: n_spans stores
}
u32 owner_list_spans(u64 n_minimizers) { return (u32)((n_minimizers + OWNL_SPAN - 1) / OWNL_SPAN); }
// list: n pairs of u32; seg: owner_list_spans(m1 - m0) + 1 entries
void launch_list_segments(const u32* list, u64 n, u32 n_spans, u32* seg, hipStream_t s) {
    (void)hipMemsetD32Async((hipDeviceptr_t)seg, (int)(u32)n, (size_t)n_spans + 1, s);
    if (n && n_spans) hipLaunchKernelGGL(list_segments_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, list, n, n_spans, seg);
}
// inserts exactly the listed windows, one workgroup per span of window starts: the span's hashes are staged in LDS once (coalesced) and
// orientation, key hash and the own side of the key comparison read them from there — a rank's share of a foreign sketch is one window in
// `world`, read straight from HBM every one of them would fetch its k values over again
static size_t listed_span_lds(const TableArgs& T) { return ((size_t)OWNL_SPAN + T.ks.k) * sizeof(u64) + OWNL_SPAN; }      // hashes + the span's claim bytes
__global__ __launch_bounds__(256) void insert_listed_span_kernel(TableArgs T, const u64* __restrict__ mh, u32* __restrict__ mread, const u64* __restrict__ roff,
                                                                 u64 m0, u64 m1, const u32* __restrict__ list, const u32* __restrict__ seg, u64 n, u32 slot0,
                                                                 u32 n_reads, u64 first_ordinal, u32* __restrict__ cap_err) {
    extern __shared__ u64 sh_keys[];           // [OWNL_SPAN + k - 1] (+ one more, then u8 cl[OWNL_SPAN]: the span's claim bytes, T.claim)
    if (cap_err[1]) return;
    const u32 q = blockIdx.x, k = T.ks.k;
    const u32 s0 = seg[q], s1 = seg[q + 1];
    const u64 b0 = m0 + (u64)q * OWNL_SPAN;
    u8* const cl = (u8*)(sh_keys + OWNL_SPAN + k);
    const u64 span_n = m1 - b0 < (u64)OWNL_SPAN ? m1 - b0 : (u64)OWNL_SPAN;      // window starts of this span that exist
    if (s0 >= s1 || s1 > n) {                      // nothing listed here: no window of this span created a key (every byte of a batch's claim map is written by somebody)
        if (T.claim) for (u32 li = threadIdx.x; li < span_n; li += 256) T.claim[b0 + li] = 0;
        return;
    }
    const u64 lim = b0 + OWNL_SPAN + k - 1 < m1 ? b0 + OWNL_SPAN + k - 1 : m1;
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    if (T.claim) for (int u = threadIdx.x; u < OWNL_SPAN / 8; u += 256) ((u64*)cl)[u] = 0;
    __syncthreads();
    for (u32 base = s0; base < s1; base += 256) {
        const u32 j = base + threadIdx.x;
        bool ok = j < s1;
        u32 li = 0; u64 i = 0;
        u32 slot = 0; u64 rs = 0;
        if (ok) {
            const uint2 e = ((const uint2*)list)[j];
            li = e.x; ok = li / OWNL_SPAN == q && e.y < n_reads; li -= q * OWNL_SPAN; i = b0 + li; slot = slot0 + e.y;
        }
        if (ok) {                                  // a wrong list is caught by the count check
            rs = roff[slot]; const u64 re = roff[slot + 1];
            ok = i >= rs && re - rs > k && i + k <= re && (!listed_check(j) || window_owner(sh_keys + li, k, OwnerSpec{T.own_world, T.own_thr}) == T.own_rank);
        }
        wave_count_add(ok, T.own_inserted);
        const u64 win = i - rs;
        if (ok && win > WIN_MASK) { *cap_err = 1; ok = false; }
        const u64 ord = ((first_ordinal + (slot - slot0)) << WIN_BITS) | win;
        bool claimed, found;
        const u64 s = upsert_wave(T, ok, li, i, sh_keys + li, k, claimed, found);      // (a wave-wide call: no lane leaves the loop early)
        if (claimed) { mread[i] = slot; if (T.claim) cl[li] = 1; }      // (mread: rep_ordinal() finds the representative's read through it; the rest of a listed batch's map is filled on demand)
        if (found) record_hit(T, s, ord);
    }
    if (T.claim) {                                 // the span's claim bytes, 64 consecutive bytes per wave and store
        __syncthreads();
        for (u32 li = threadIdx.x; li < span_n; li += 256) T.claim[b0 + li] = cl[li];
    }
}
// Few listed windows per span (a rank's share of a sketch at 4+ ranks): staging every span of the sketch would mostly fetch hashes nobody needs, and
// a workgroup would work off a few dozen entries; the per-entry kernel reads each window's values where they lie.  So do very long k (the span does not
// fit the default LDS window) and a list without segments.
constexpr u64 LISTED_SPAN_MIN = 150;          // listed windows per span below which a batch takes the per-entry kernel
// true: launch_insert_listed takes the per-entry kernel for this batch (then several such batches can share one launch, launch_insert_listed_multi, and their
// claim bytes must start from zero: the per-entry kernel sets only the byte of a window that creates its key, the span kernel writes every byte of its batch)
bool listed_per_entry(const TableArgs& T, u64 m0, u64 m1, u64 n, bool have_seg) {
    return !have_seg || listed_span_lds(T) > 64 * 1024 || n < (u64)owner_list_spans(m1 - m0) * LISTED_SPAN_MIN;
}
// list: n pairs (window start, read), seg: launch_list_segments of it
void launch_insert_listed(const TableArgs& T, const u64* mh, u32* mread, const u64* roff, u64 m0, u64 m1, const u32* list, const u32* seg, u64 n, u32 slot0,
                          u32 n_reads, u64 first_ordinal, u32* cap_err, hipStream_t s) {
    if (!n) return;
    if (!listed_per_entry(T, m0, m1, n, seg != nullptr))
        hipLaunchKernelGGL(insert_listed_span_kernel, dim3(owner_list_spans(m1 - m0)), dim3(256), listed_span_lds(T), s, T, mh, mread, roff, m0, m1, list, seg, n, slot0, n_reads, first_ordinal, cap_err);
    else
        launch_listed_entries(T, mh, mread, roff, m0, m1, list, n, slot0, n_reads, first_ordinal, cap_err, nullptr, 0u, s);
}
void launch_insert_listed_multi(const TableArgs& T, const u64* mh, u32* mread, const u64* roff, const ListedBatch* d_batches, u32 n_batches, u64 total, u32* cap_err, hipStream_t s) {
    if (!total) return;
    launch_listed_entries(T, mh, mread, roff, 0ull, 0ull, nullptr, total, 0u, 0u, 0ull, cap_err, d_batches, n_batches, s);
}
