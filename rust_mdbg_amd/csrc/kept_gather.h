// kept_gather.h — device helpers of the kernels that gather bases out of the resident read store (KeptDesc, contigs.h): stitch_kernel (contigs.hip) and
// node_seq_kernel (node_seqs.hip).  One copy of the batch lookup, the span check, the per-byte read, the 16-code expansion with its exception patch and
// utils::revcomp's byte map.  Device code only; included after graph_common.h's typedefs.
#pragma once
#include "contigs.h"
#include "graph_common.h"

namespace {

enum { ERR_NOT_KEPT = 1u, ERR_OUTSIDE = 2u };      // bits of the error flag both kernels set

// src/utils.rs:10-24, as mdbg_emit.cpp's switch_base
__device__ inline u8 switch_base_dev(u8 c) {
    switch (c) { case 'a': return 't'; case 'c': return 'g'; case 't': return 'a'; case 'g': return 'c'; case 'u': return 'a';
                 case 'A': return 'T'; case 'C': return 'G'; case 'T': return 'A'; case 'G': return 'C'; case 'U': return 'A'; default: return 'N'; }
}
__device__ inline u8 through_revcomp(u8 c, u32 rc) { return rc == 0 ? c : rc == 1 ? switch_base_dev(c) : switch_base_dev(switch_base_dev(c)); }

// largest i in [lo, hi) with a[i] <= v; the caller knows that hi > lo (a[lo] > v is reported by the caller's own test)
__device__ inline u64 last_le(const u64* __restrict__ a, u64 lo, u64 hi, u64 v) {
    while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (a[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}

// the kept batch that holds read ordinal r (tab: sorted by first_ordinal); nullptr: the read is not kept
__device__ inline const KeptDesc* kept_batch_of(const KeptDesc* __restrict__ tab, u32 n_tab, u64 r) {
    if (n_tab == 0 || tab[0].first_ordinal > r) return nullptr;
    u32 lo = 0, hi = n_tab;
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (tab[mid].first_ordinal <= r) lo = mid; else hi = mid; }
    const KeptDesc* const d = tab + lo;
    return r - d->first_ordinal < d->n_reads ? d : nullptr;
}
// bases [b, b + n) of read r of batch d -> *sb = position of the first of them in the batch; false: they do not lie inside the read (nothing may be read)
__device__ inline bool kept_span(const KeptDesc* d, u64 r, u64 b, u64 n, u64* sb) {
    const u64 rl = r - d->first_ordinal;
    const u64 ro = d->offsets[rl], re = d->offsets[rl + 1];
    if (re < ro || re > d->n_words * 32 || b > re - ro || n > re - ro - b) return false;
    *sb = ro + b;
    return true;
}
// the original byte at position q of a kept batch
__device__ inline u8 kept_byte(const KeptDesc* d, u64 q) {
    if (d->n_exc) {
        const u64* const xp = d->exc_pos;
        u64 lo = 0, hi = d->n_exc;
        while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (xp[mid] < q) lo = mid + 1; else hi = mid; }
        if (lo < d->n_exc && xp[lo] == q) return d->exc_val[lo];
    }
    const uint2 w = d->planes[q >> 5];
    const u32 b = (u32)q & 31u;
    const u32 code = ((w.x >> b) & 1u) | (((w.y >> b) & 1u) << 1);
    return (u8)(0x47544341u >> (8 * code));          // "ACTG"
}
// The 16 bytes at positions [qs, qs + 16) of a kept batch (the caller has checked that they lie inside one read), as 16 output bytes: in source order, or
// reverse-complemented (rev: the 16 codes are taken in one piece, bit-reversed, and the high plane flipped — the complement of code c is c ^ 2).  Bytes the
// planes cannot hold come from the exception side-list, through utils::revcomp's map rc times; the patch runs only in batches that have exceptions.
__device__ inline uint4 kept_group16(const KeptDesc* d, u64 qs, bool rev, u32 rc) {
    const u64 w = qs >> 5; const u32 b = (u32)qs & 31u;
    const uint2 w0 = d->planes[w];
    uint2 w1 = make_uint2(0, 0);
    if (b > 16 && w + 1 < d->n_words) w1 = d->planes[w + 1];
    u32 lo = (u32)((((u64)w1.x << 32) | w0.x) >> b) & 0xFFFFu, hi = (u32)((((u64)w1.y << 32) | w0.y) >> b) & 0xFFFFu;
    if (rev) { lo = __brev(lo) >> 16; hi = (__brev(hi) >> 16) ^ 0xFFFFu; }
    u32 o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        u32 v = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = 4 * q + t;
            const u32 code = ((lo >> j) & 1u) | (((hi >> j) & 1u) << 1);
            v |= ((0x47544341u >> (8 * code)) & 0xFFu) << (8 * t);
        }
        o[q] = v;
    }
    uint4 ov = make_uint4(o[0], o[1], o[2], o[3]);
    if (d->n_exc) {                                  // rare: patch the bytes the planes cannot hold
        const u64* const xp = d->exc_pos;
        u64 i = 0, hi_i = d->n_exc;
        while (i < hi_i) { const u64 mid = i + ((hi_i - i) >> 1); if (xp[mid] < qs) i = mid + 1; else hi_i = mid; }
        for (; i < d->n_exc && xp[i] < qs + 16; ++i) {
            const u32 j = rev ? 15u - (u32)(xp[i] - qs) : (u32)(xp[i] - qs);
            const u32 v = through_revcomp(d->exc_val[i], rc), sh = 8 * (j & 3u), m = ~(0xFFu << sh);
            const u32 q = j >> 2;
            if (q == 0) ov.x = (ov.x & m) | (v << sh); else if (q == 1) ov.y = (ov.y & m) | (v << sh);
            else if (q == 2) ov.z = (ov.z & m) | (v << sh); else ov.w = (ov.w & m) | (v << sh);
        }
    }
    return ov;
}

}  // namespace
