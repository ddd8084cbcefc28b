// dev_util.hip — small device helpers that belong to no stage (gfx950): zeroing and filling, folding the sharded counters, publishing the scalars the host reads,
// the read map and the read offsets of an imported region.  Included ahead of table.hip: clear_table_kernel takes a ZeroList.
#include "mdbg_dev.h"
struct ZeroList { u64* p[6]; u64 n[6]; u64* set_p; u64 set_v; };
// Several small regions zeroed (and one scalar set) by ONE launch: the steps between the big kernels would otherwise be chains of
// 5-microsecond fill kernels (ten of them in front of the sketch, five in front of finalize).
__global__ __launch_bounds__(256) void zero_regions_kernel(ZeroList z) {
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x, stride = (u64)gridDim.x * blockDim.x;
#pragma unroll
    for (int r = 0; r < 6; ++r) for (u64 i = i0; i < z.n[r]; i += stride) z.p[r][i] = 0;
    if (i0 == 0 && z.set_p) *z.set_p = z.set_v;
}
void launch_zero_regions(const ZeroList& z, hipStream_t s) {
    u64 mx = 1;
    for (int r = 0; r < 6; ++r) mx = z.n[r] > mx ? z.n[r] : mx;
    const unsigned blocks = (unsigned)std::min<u64>(1024, (mx + 255) / 256);
    hipLaunchKernelGGL(zero_regions_kernel, dim3(blocks), dim3(256), 0, s, z);
}
__global__ __launch_bounds__(256) void fill_u64_kernel(u64* __restrict__ p, u64 n, u64 v) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) p[i] = v;
}
void launch_fill_u64(u64* p, u64 n, u64 v, hipStream_t s) {
    if (n) hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)std::min<u64>(1024, (n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

// out[j] = sum of shard array j (CTR_SHARDS u64 each); one block per array
__global__ __launch_bounds__(256) void sum_shards_kernel(const u64* __restrict__ shards, u64* __restrict__ out) {
    __shared__ u64 ws[4];
    const u64* s = shards + (size_t)blockIdx.x * CTR_SHARDS;
    u64 v = 0;
    for (int i = threadIdx.x; i < CTR_SHARDS; i += 256) v += s[i];
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
void launch_sum_shards(const u64* shards, u32 n_arrays, u64* out, hipStream_t s) {
    hipLaunchKernelGGL(sum_shards_kernel, dim3(n_arrays), dim3(256), 0, s, shards, out);
}

// What the host reads between the stages, in one launch: scalars[idx[j]] = sum of shard array j (up to three), then all n scalars -> pinned
// host memory (was: the sum kernels, a copy kernel and the runtime's staging of a pageable destination in front of every host decision).
// host[n] = seq is written last (system-scope fence in between): the host polls that word instead of waiting for the queue's completion signal
struct PublishArgs { const u64* shards[3]; u32 idx[3]; u32 n_arrays; u64* scalars; u32 n; u32 zero_idx; u64* host; u64 seq;      // zero_idx: scalar reset once it has been published (>= n: none)
                     u64 zero_mask; u32 zero_arrays; };      // zero_mask: further scalars reset behind the copy (bit i: scalar i); zero_arrays: bit j: shard array j is zeroed once it has been summed
                                                              // (the finalize counters are left clean for the next finalize: no zeroing launch in front of it)
__global__ __launch_bounds__(1024) void publish_scalars_kernel(PublishArgs p) {
    __shared__ u64 ws[3][16];
    static_assert(CTR_SHARDS % 1024 == 0, "whole rounds");
    for (u32 j = 0; j < p.n_arrays; ++j) {
        u64 v = 0;
#pragma unroll
        for (int i = 0; i < CTR_SHARDS / 1024; ++i) v += p.shards[j][threadIdx.x + 1024 * i];
        if ((p.zero_arrays >> j) & 1u) for (int i = 0; i < CTR_SHARDS / 1024; ++i) ((u64*)p.shards[j])[threadIdx.x + 1024 * i] = 0;      // (every entry is read and zeroed by the same thread)
        for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0) ws[j][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < p.n) {
        u64 v = p.scalars[threadIdx.x];
        for (u32 j = 0; j < p.n_arrays; ++j) if (threadIdx.x == p.idx[j]) { v = 0; for (int q = 0; q < 16; ++q) v += ws[j][q]; p.scalars[threadIdx.x] = v; }
        __hip_atomic_store(p.host + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (threadIdx.x == p.zero_idx || ((p.zero_mask >> threadIdx.x) & 1ull)) p.scalars[threadIdx.x] = 0;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(p.host + p.n, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_publish_scalars(const PublishArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(publish_scalars_kernel, dim3(1), dim3(1024), 0, s, p);
}

// imported sketches: mread[i] = slot of the read minimizer i belongs to (one wave per read)
__global__ __launch_bounds__(256) void fill_mread_kernel(const u64* __restrict__ roff, u32 slot0, u32 n_reads, u32* __restrict__ mread) {
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const u64 a = roff[slot0 + r], b = roff[slot0 + r + 1];
    for (u64 i = a + (threadIdx.x & 63); i < b; i += 64) mread[i] = slot0 + r;
}
void launch_fill_mread(const u64* roff, u32 slot0, u32 n_reads, u32* mread, hipStream_t s) {
    if (n_reads) hipLaunchKernelGGL(fill_mread_kernel, dim3((n_reads + 3) / 4), dim3(256), 0, s, roff, slot0, n_reads, mread);
}
// roff[slot0 + r] = m0 + rel[r] for r in [0, n_reads]
__global__ void rebase_offsets_kernel(const u64* __restrict__ rel, u32 n_reads, u64 m0, u64* __restrict__ roff_out) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= n_reads) roff_out[r] = m0 + rel[r];
}
void launch_rebase_offsets(const u64* rel, u32 n_reads, u64 m0, u64* roff_out, hipStream_t s) {
    hipLaunchKernelGGL(rebase_offsets_kernel, dim3((n_reads + 256) / 256), dim3(256), 0, s, rel, n_reads, m0, roff_out);
}

// same for an imported region, with the caller's offsets checked on the device: [0] = 0, non-decreasing, [n_reads] = n_min
__global__ void rebase_offsets_checked_kernel(const u64* __restrict__ rel, u32 n_reads, u64 m0, u64 n_min, u64* __restrict__ roff_out, u64* __restrict__ bad) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    const u64 v = rel[r];
    if (v > n_min || (r == 0 && v != 0) || (r == n_reads && v != n_min) || (r < n_reads && rel[r + 1] < v)) *bad = 1;
    roff_out[r] = m0 + (v > n_min ? n_min : v);
}
void launch_rebase_offsets_checked(const u64* rel, u32 n_reads, u64 m0, u64 n_min, u64* roff_out, u64* bad, hipStream_t s) {
    hipLaunchKernelGGL(rebase_offsets_checked_kernel, dim3((n_reads + 256) / 256), dim3(256), 0, s, rel, n_reads, m0, n_min, roff_out, bad);
}
