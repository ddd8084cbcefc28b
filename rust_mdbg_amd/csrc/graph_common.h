// graph_common.h — what the graph stages (edges.hip, unitigs.hip, simplify.hip, contigs.hip, placement.hip, ...) share on the host side: the grow-only device block, the
// two-phase rocPRIM calls, the read-back of a scan's total and the timer of a read-evidence stage.  Header-only; it pulls in rocPRIM, so only those translation units include it (never libmdbg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

typedef uint8_t u8; typedef uint16_t u16; typedef uint32_t u32; typedef uint64_t u64;

// Device memory of the library comes from a process-wide cache of blocks (api.inc): hipMalloc after large frees takes SECONDS on this stack
// (the driver releases memory lazily and the next allocation waits for it: profiles/r04_c_alloc_trace.txt), so freed blocks of 1 MB and more
// are kept and handed out again.  *cap <- usable size (>= bytes).
hipError_t mdbg_block_alloc(void** p, size_t bytes, size_t* cap);
void mdbg_block_free(void* p, size_t cap);
// MDBG_GUARD (test hook, blocks.inc): every block is handed out exactly as large as it was asked for, between two bands that are checked for writes; whoever adds slack to a request asks this first
__attribute__((visibility("hidden"))) bool mdbg_guard_mode();

// the one error convention of the graph stages: every host function returns the failing HIP error (a broken invariant has its own out-parameter, unitigs.h)
#define GHIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

namespace {

// grow-only device block; growing does not keep the contents
struct Buf {
    void* p = nullptr; size_t cap = 0;
    ~Buf() { if (p) mdbg_block_free(p, cap); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) mdbg_block_free(p, cap);
        p = nullptr; cap = 0;
        return mdbg_block_alloc(&p, mdbg_guard_mode() ? bytes : bytes + bytes / 8 + 256, &cap);
    }
    template <class T> T* as() const { return (T*)p; }
};

inline unsigned grid_for(u64 n) { return (unsigned)((n + 255) / 256); }

// device time of one call of a read-evidence stage (read_paths.hip, junctions.hip, transits.hip), and how such a call ends
struct StageTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~StageTimer() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
    hipError_t start(hipStream_t s) {
        if (!ev0) { GHIP(hipEventCreate(&ev0)); GHIP(hipEventCreate(&ev1)); }
        return hipEventRecord(ev0, s);
    }
    // the closing event, ONE read-back (the stage's counters) and the call's ONE wait; *ms <- device time since start()
    hipError_t stop_and_read(void* host, const void* dev, size_t bytes, hipStream_t s, float* ms) {
        GHIP(hipEventRecord(ev1, s));
        GHIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
        GHIP(hipStreamSynchronize(s));
        if (hipEventElapsedTime(ms, ev0, ev1) != hipSuccess) { (void)hipGetLastError(); *ms = 0; }
        return hipSuccess;
    }
};

// ---- rocPRIM, two-phase: ask for the temporary size, grow `tmp`, run.  One `tmp` serves every call of a stage although the calls are only stream-ordered:
// growing it frees the old block through mdbg_block_free, which synchronises the device for blocks of 1 MB and more, and hipFree does so for smaller ones,
// so whatever still works in the old block is over before anybody else can get it.
template <class In, class Out>
hipError_t excl_scan(Buf& tmp, const In* in, Out* out, size_t n, hipStream_t s) {
    size_t tb = 0;
    GHIP(rocprim::exclusive_scan(nullptr, tb, in, out, (Out)0, n, rocprim::plus<Out>(), s));
    GHIP(tmp.ensure(tb + 256));
    return rocprim::exclusive_scan(tmp.p, tb, in, out, (Out)0, n, rocprim::plus<Out>(), s);
}
// (the sorts take their pointers as the caller has them, const or not: the rocPRIM instantiation is the caller's)
template <class KeyIn, class KeyOut>
hipError_t sort_keys(Buf& tmp, KeyIn in, KeyOut out, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
    size_t tb = 0;
    GHIP(rocprim::radix_sort_keys(nullptr, tb, in, out, n, begin_bit, end_bit, s));
    GHIP(tmp.ensure(tb + 256));
    return rocprim::radix_sort_keys(tmp.p, tb, in, out, n, begin_bit, end_bit, s);
}
template <class KeyIn, class KeyOut, class ValIn, class ValOut>      // stable
hipError_t sort_pairs(Buf& tmp, KeyIn kin, KeyOut kout, ValIn vin, ValOut vout, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
    size_t tb = 0;
    GHIP(rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, n, begin_bit, end_bit, s));
    GHIP(tmp.ensure(tb + 256));
    return rocprim::radix_sort_pairs(tmp.p, tb, kin, kout, vin, vout, n, begin_bit, end_bit, s);
}
// every segment [offsets[i], offsets[i + 1]) on its own
template <class KeyIn, class KeyOut>
hipError_t sort_segments(Buf& tmp, KeyIn in, KeyOut out, unsigned n, unsigned n_segments, const u32* offsets, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
    size_t tb = 0;
    GHIP(rocprim::segmented_radix_sort_keys(nullptr, tb, in, out, n, n_segments, offsets, offsets + 1, begin_bit, end_bit, s));
    GHIP(tmp.ensure(tb + 256));
    return rocprim::segmented_radix_sort_keys(tmp.p, tb, in, out, n, n_segments, offsets, offsets + 1, begin_bit, end_bit, s);
}

// total of an exclusive scan over n > 0 elements = last input + last output.  scan_total queues the two read-backs on the stream and does NOT wait: the caller
// synchronises once for everything it has queued (several totals, other counters) and reads total() afterwards.
template <class In, class Out> struct ScanLast { In in{}; Out out{}; u64 total() const { return (u64)in + (u64)out; } };
template <class In, class Out>
hipError_t scan_total(const In* in, const Out* out, size_t n, hipStream_t s, ScanLast<In, Out>* last) {
    GHIP(hipMemcpyAsync(&last->in, in + (n - 1), sizeof(In), hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(&last->out, out + (n - 1), sizeof(Out), hipMemcpyDeviceToHost, s);
}

}  // namespace
