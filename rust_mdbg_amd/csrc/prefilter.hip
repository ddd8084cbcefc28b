// prefilter.hip — the counting pre-filter in front of the node table (MDBG_FLAG_PREFILTER; include/mdbg_hip.h has the definition): two bits per cell, a counter that
// saturates at 2, over ALL windows of the resident batches; a window enters the table only when its cell has been hit twice (gfx950).  Needs table.hip (orientation,
// key hash, OWN_SPAN).
//
// Both kernels are shaped like insert_windows_kernel: one workgroup per OWN_SPAN window starts, the span's OWN_SPAN + k - 1 hashes staged in LDS once, orientation and
// key hash read from there; a window start counts only if its read has more than k minimizers and the window ends inside it.
#include "mdbg_dev.h"

constexpr u64 PF_SALT = 0x9E3779B97F4A7C15ull;
constexpr u64 PF_DEFAULT_CELLS = 1ull << 32, PF_MAX_CELLS = 1ull << 36;
// cell of a key hash; 16 cells per 32-bit word, cell c in bits [2 (c & 15), 2 (c & 15) + 2): 00 never seen, 01 seen once, 11 seen twice or more
__device__ inline u64 prefilter_cell(u64 h, u64 n_cells) { return __umul64hi(fmix64(h ^ PF_SALT), n_cells); }
static size_t prefilter_words(u64 n_cells) { return (size_t)((n_cells + 15) / 16); }
static size_t prefilter_lds(u32 k) { return ((size_t)OWN_SPAN + k) * sizeof(u64); }

// stages the span's hashes; returns through b0 the span's first index.  All 256 threads call it.
__device__ inline void prefilter_stage(u64* sh_keys, const u64* __restrict__ mh, u64 i0, u64 i1, u32 k, u64& b0) {
    b0 = i0 + (u64)blockIdx.x * OWN_SPAN;
    const u64 lim = b0 + OWN_SPAN + k - 1 < i1 ? b0 + OWN_SPAN + k - 1 : i1;
    for (u64 t = b0 + threadIdx.x; t < lim; t += 256) sh_keys[t - b0] = mh[t];
    __syncthreads();
}
// does a window start at index i (span position li), and in which cell does it fall?
__device__ inline bool prefilter_window(const u64* sh_keys, u32 li, u64 i, u64 i1, u32 k, const u32* __restrict__ mread, const u64* __restrict__ roff, u64 n_cells, u64& cell) {
    if (i + k > i1) return false;
    const u32 slot = mread[i];
    const u64 rs = roff[slot], re = roff[slot + 1];
    if (!(re - rs > k && i + k <= re)) return false;
    const u64* w = sh_keys + li;
    const bool rev = window_reversed(w, k);
    cell = prefilter_cell(key_hash_window(w, k, rev), n_cells);
    return true;
}

// Every window of the minimizers [i0, i1) of a batch bumps its cell.  A plain load first: a cell that reads 2 already is left alone (most windows of real data are
// repeats of solid keys).  Else a relaxed agent-scope fetch_or of the low bit, and when the old value had it, a second one of the high bit.  Cell states only grow, so a
// stale plain read costs one redundant atomic and never a wrong state: the cell ends at min(2, arrivals) whatever their order.
__global__ __launch_bounds__(256) void prefilter_count_kernel(u32* __restrict__ cells, u64 n_cells, const u64* __restrict__ mh, const u32* __restrict__ mread,
                                                              const u64* __restrict__ roff, u64 i0, u64 i1, u32 k) {
    extern __shared__ u64 sh_keys[];
    u64 b0;
    prefilter_stage(sh_keys, mh, i0, i1, k, b0);
#pragma unroll 1
    for (int u = 0; u < OWN_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        u64 cell = 0;
        if (!prefilter_window(sh_keys, li, b0 + li, i1, k, mread, roff, n_cells, cell)) continue;
        u32* const wp = cells + (cell >> 4);
        const u32 sh = (u32)(cell & 15) * 2;
        if ((*wp >> sh) & 2u) continue;
        const u32 old = __hip_atomic_fetch_or(wp, 1u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old >> sh) & 1u) __hip_atomic_fetch_or(wp, 2u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
void launch_prefilter_count(u32* cells, u64 n_cells, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, hipStream_t s) {
    if (i1 <= i0) return;
    hipLaunchKernelGGL(prefilter_count_kernel, dim3((unsigned)((i1 - i0 + OWN_SPAN - 1) / OWN_SPAN)), dim3(256), prefilter_lds(k), s, cells, n_cells, mh, mread, roff, i0, i1, k);
}

// After ALL counting: one admission bit per window start of the batch — bit (i - i0) of adm[] is set when a window starts at i and its cell reads 2 — one 64-bit word per
// wave from a ballot, stored by one lane; adm[] has (i1 - i0 + 63) / 64 words and every one of them is written.  The admitted windows are added to the sharded counter
// `admitted` (one atomic per wave, as wave_count_add): the sum sizes the table.
__global__ __launch_bounds__(256) void prefilter_admit_kernel(const u32* __restrict__ cells, u64 n_cells, const u64* __restrict__ mh, const u32* __restrict__ mread,
                                                              const u64* __restrict__ roff, u64 i0, u64 i1, u32 k, u64* __restrict__ adm, u64* __restrict__ admitted) {
    extern __shared__ u64 sh_keys[];
    u64 b0;
    prefilter_stage(sh_keys, mh, i0, i1, k, b0);
#pragma unroll 1
    for (int u = 0; u < OWN_SPAN / 256; ++u) {
        const u32 li = u * 256 + threadIdx.x;
        const u64 i = b0 + li;
        u64 cell = 0;
        bool ok = prefilter_window(sh_keys, li, i, i1, k, mread, roff, n_cells, cell);
        if (ok) ok = ((cells[cell >> 4] >> ((u32)(cell & 15) * 2)) & 2u) != 0;
        const u64 m = __ballot(ok);
        const u64 w0 = i - (threadIdx.x & 63);                 // the wave's first index: b0 - i0 is a multiple of OWN_SPAN, so a wave is one word of adm[]
        if ((threadIdx.x & 63) == 0 && w0 < i1) {
            adm[(w0 - i0) >> 6] = m;
            if (m) atomicAdd((unsigned long long*)ctr_shard(admitted), (unsigned long long)__popcll(m));
        }
    }
}
void launch_prefilter_admit(const u32* cells, u64 n_cells, const u64* mh, const u32* mread, const u64* roff, u64 i0, u64 i1, u32 k, u64* adm, u64* admitted, hipStream_t s) {
    if (i1 <= i0) return;
    hipLaunchKernelGGL(prefilter_admit_kernel, dim3((unsigned)((i1 - i0 + OWN_SPAN - 1) / OWN_SPAN)), dim3(256), prefilter_lds(k), s, cells, n_cells, mh, mread, roff, i0, i1, k, adm, admitted);
}
