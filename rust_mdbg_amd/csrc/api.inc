// api.inc — context management and the C ABI of include/mdbg_hip.h (host code; included by libmdbg.hip
// after sketch.hip / table.hip / synth.hip so that it sees their launchers and argument structs).
#include <algorithm>
#include <cstdio>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mdbg_hip.h"
#include "edges.h"
#include "unitigs.h"
#include "simplify.h"
#include "contigs.h"

namespace {


constexpr u64 SLAB_BUDGET = 6ull << 30;       // bytes of per-tile slabs per sketch launch (denser settings run in several launches)

// MDBG_ALLOC_TRACE=<file>: one line per (re)allocation of 16 MB or more with the time of each runtime call (diagnostic)
inline FILE* alloc_trace() { static FILE* const f = [] { const char* p = getenv("MDBG_ALLOC_TRACE"); return p ? fopen(p, "a") : (FILE*)nullptr; }(); return f; }
inline double now_ms() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
// ---- process-wide cache of device blocks ------------------------------------------------------------------------------------------
// Measured (profiles/r04_c_alloc_trace.txt): a hipMalloc that follows large hipFree calls takes 1 - 5 SECONDS whatever its size (24 GB: 2.7 s,
// 1.3 GB: 3.2 s) — the frees return at once and the next allocation pays for them.  A context that grows its sketch store or its table, a host
// that runs several contexts one after the other, and the test suite (10 of the 14 seconds of the streamed full-size test) all met it.
// So blocks of 1 MB and more are never handed back to the runtime while the process lives and the cache holds less than its cap: a request
// takes the smallest cached block of its device that fits and is at most twice as large; hipMalloc is the fallback, and when that runs out of
// memory the cache is emptied and it is tried again.  MDBG_CACHE_MB (default: a third of the device) caps the cached bytes PER DEVICE, 0 switches the cache off;
// mdbg_release_cached_memory() empties it.  The emptying on out-of-memory only helps the library's OWN allocations: a host with another device allocator in the
// process (torch's caching allocator, RCCL, its own hipMalloc) sees the cached bytes as used memory — INTEGRATION.md tells it to call
// mdbg_release_cached_memory() after destroying its contexts or to set MDBG_CACHE_MB.
struct BlockCache {
    struct Blk { void* p; size_t cap; int dev; };
    static constexpr int MAX_DEV = 64;
    std::mutex mu; std::vector<Blk> blocks; size_t bytes = 0;
    size_t dev_bytes[MAX_DEV] = {}, dev_limit[MAX_DEV] = {}; bool dev_known[MAX_DEV] = {};       // the cap is PER DEVICE: a third of THAT device (or MDBG_CACHE_MB each)
    static constexpr size_t MIN_BLOCK = 1u << 20;
    size_t cap_limit(int dev) {                // (mu held)
        const int d = dev >= 0 && dev < MAX_DEV ? dev : 0;
        if (!dev_known[d]) {
            dev_known[d] = true;
            const char* e = getenv("MDBG_CACHE_MB");
            if (e) dev_limit[d] = (size_t)strtoull(e, nullptr, 10) << 20;
            else { size_t tot = 0; dev_limit[d] = hipDeviceTotalMem(&tot, dev) == hipSuccess ? tot / 3 : (size_t)64 << 30; (void)hipGetLastError(); }
        }
        return dev_limit[d];
    }
    void* take(size_t need, int dev, size_t* cap) {
        std::lock_guard<std::mutex> g(mu);
        size_t best = ~(size_t)0;
        for (size_t i = 0; i < blocks.size(); ++i) {
            const Blk& b = blocks[i];
            if (b.dev == dev && b.cap >= need && b.cap <= 2 * need + (MIN_BLOCK << 3) && (best == ~(size_t)0 || b.cap < blocks[best].cap)) best = i;
        }
        if (best == ~(size_t)0) return nullptr;
        void* p = blocks[best].p; *cap = blocks[best].cap; bytes -= blocks[best].cap; dev_bytes[dev >= 0 && dev < MAX_DEV ? dev : 0] -= blocks[best].cap;
        blocks[best] = blocks.back(); blocks.pop_back();
        return p;
    }
    bool give(void* p, size_t cap, int dev) {
        std::lock_guard<std::mutex> g(mu);
        const int d = dev >= 0 && dev < MAX_DEV ? dev : 0;
        if (cap < MIN_BLOCK || dev_bytes[d] + cap > cap_limit(dev)) return false;
        blocks.push_back(Blk{p, cap, dev}); bytes += cap; dev_bytes[d] += cap;
        return true;
    }
    size_t trim() {
        std::vector<Blk> out;
        { std::lock_guard<std::mutex> g(mu); out.swap(blocks); bytes = 0; for (size_t& b : dev_bytes) b = 0; }
        size_t n = 0; int cur = 0; (void)hipGetDevice(&cur);
        for (const Blk& b : out) { if (b.dev != cur) (void)hipSetDevice(b.dev); (void)hipFree(b.p); if (b.dev != cur) (void)hipSetDevice(cur); n += b.cap; }
        return n;
    }
};
inline BlockCache& block_cache() { static BlockCache* const c = new BlockCache(); return *c; }     // (never destroyed: blocks may be returned by static destructors)
}  // namespace
hipError_t mdbg_block_alloc(void** p, size_t bytes, size_t* cap) {
    int dev = 0; (void)hipGetDevice(&dev);
    const double t0 = now_ms();
    bool cached = true;
    void* q = bytes >= BlockCache::MIN_BLOCK ? block_cache().take(bytes, dev, cap) : nullptr;
    if (!q) {
        cached = false;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); if (block_cache().trim()) e = hipMalloc(&q, bytes); }
        if (e != hipSuccess) return e;
        *cap = bytes;
    }
    if (alloc_trace() && bytes >= (16u << 20)) { fprintf(alloc_trace(), "alloc bytes=%zu cap=%zu %s %.3f ms\n", bytes, *cap, cached ? "cache" : "hipMalloc", now_ms() - t0); fflush(alloc_trace()); }
    // MDBG_POISON (test hook): every block is handed out filled with 0xA5, so that nothing can lean on the zeros a fresh hipMalloc happens to deliver
    static const bool poison = getenv("MDBG_POISON") != nullptr;
    if (poison) {        // (the fill runs on the null stream, which the contexts' non-blocking streams do not wait for: it has to be over before anybody writes the block)
        if (hipMemset(q, 0xA5, *cap) != hipSuccess) (void)hipGetLastError();
        (void)hipDeviceSynchronize();
    }
    *p = q;
    return hipSuccess;
}
void mdbg_block_free(void* p, size_t cap) {
    if (!p) return;
    int dev = 0; (void)hipGetDevice(&dev);
    // what hipFree guarantees and the callers rely on: nothing on the device still uses the block when somebody else gets it
    if (cap >= BlockCache::MIN_BLOCK) (void)hipDeviceSynchronize();
    if (!block_cache().give(p, cap, dev)) (void)hipFree(p);
}
namespace {
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    ~DevBuf() { release(); }
    // grow to at least `bytes`; keep = number of leading bytes to preserve
    hipError_t ensure(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        size_t ncap = 0;
        void* np = nullptr;
        hipError_t e = mdbg_block_alloc(&np, bytes + bytes / 4 + 256, &ncap);
        if (e != hipSuccess) { (void)hipGetLastError(); e = mdbg_block_alloc(&np, bytes + 256, &ncap); if (e != hipSuccess) return e; }
        if (p && keep) { e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, s); if (e != hipSuccess) { mdbg_block_free(np, ncap); return e; } (void)hipStreamSynchronize(s); }
        if (p) mdbg_block_free(p, cap);      // (every user of the old block was ordered before the copy or is done: callers grow a buffer only between its uses)
        p = np; cap = ncap;
        return hipSuccess;
    }
    void release() { if (p) mdbg_block_free(p, cap); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// One batch of the resident read store (MDBG_FLAG_KEEP_READS): the packed layout of mdbg_packed_batch in device blocks of its own — `blk` holds the planes
// (n_words x 8 bytes) followed by the n_reads + 1 offsets, `xblk` (only when there are exceptions) the n_exc positions followed by the n_exc bytes.
// Owned by its Batch, so it lives exactly as long as the batch's sketch does (mdbg_reset(0) and mdbg_rewind drop both).
struct KeptReads {
    void* blk = nullptr; size_t cap = 0; void* xblk = nullptr; size_t xcap = 0;
    u64 n_reads = 0, n_bases = 0, n_words = 0, n_exc = 0;
    KeptReads() = default; KeptReads(const KeptReads&) = delete; KeptReads& operator=(const KeptReads&) = delete;
    ~KeptReads() { if (blk) mdbg_block_free(blk, cap); if (xblk) mdbg_block_free(xblk, xcap); }
    uint2* planes() const { return (uint2*)blk; }
    u64* offsets() const { return (u64*)blk + n_words; }
    u64* exc_pos() const { return (u64*)xblk; }
    u8* exc_val() const { return (u8*)xblk + n_exc * 8; }
    u64 bytes() const { return n_words * 8 + (n_reads + 1) * 8 + n_exc * 9; }
};
struct Batch { u64 first_ordinal; u32 n_reads; u32 slot0; u64 m0, m1; u64 owned = ~0ull;    // owned: windows of the batch this rank owns, if known
               u64 list_off = ~0ull;                                                       // their list (mdbg_owner_lists): offset into mdbg_ctx::own_lists, `owned` pairs + segments
               bool mread_ok = true;
               u32 src_rank = ~0u;                                                          // sketch exchange: the rank that sketched the batch (~0: this context); its positions are NOT resident when set
               u64 n_bases = 0;
               bool partial = false;
               std::shared_ptr<KeptReads> kept; };                                                    // a foreign sketch of which only the hashes of this rank's listed windows are resident (mdbg_dist, segments)                                                         // raw bases of the batch (0: imported sketch)                                                    // false: imported with a list, the minimizer -> read map is filled on demand (ensure_mread)

// shard arrays (CTR_SHARDS u64 each): SH_DISTINCT keys in the table; SH_OWNED / SH_OWNINS: windows a partitioned context owns / inserted (zeroed by their users);
// SH_FIN_WRAPPED / SH_FIN_DISTINCT: finalize's counters — touched by nothing else, and left ZERO by the finalize that used them (the kernel that publishes them
// zeroes them: read_scalars(with_fin)), so that no zeroing launch stands in front of the next finalize (mdbg_ctx::fin_dirty says when that does not hold)
enum { SH_DISTINCT = 0, SH_OWNED, SH_OWNINS, SH_FIN_WRAPPED, SH_FIN_DISTINCT, N_SHARD_ARRAYS };
// scalars[] layout (u64 each) in one small device buffer
enum { SC_CARRY = 0, SC_NDISTINCT, SC_NWINDOWS, SC_FIN0, SC_FIN1, SC_FIN2, SC_SLOWCOUNT /*u32*/, SC_ERRFLAG /*u32*/, SC_CAPERR /*u32*/, SC_SLOWTOTAL, SC_BATCHWIN, SC_IMPORTERR, SC_PROBEERR /*u32*/, SC_OWNINS, SC_OVERMAX /*u32*/, SC_TOTFIRST, SC_TOTSOLID, SC_SLICEFAIL, SC_DONE /*u32: count_reserve_kernel's workgroup counter, zero between launches*/, SC_N };

}  // namespace

// host batches are staged in one of two device buffers, each with its own copy stream: while one caller's batch is
// being sketched (context lock held), another caller's PCIe copy proceeds
struct Stage { DevBuf bases, off, exc_pos, exc_val; hipStream_t st = nullptr; bool busy = false; };
// host side of a copy-out: grown, never zero-filled (std::vector::resize wrote 150 MB of zeros under the 150-MB copy of a 465 k-node table: 25 ms of a 190-ms
// file -> .gfa run), never shrunk
template <class T> struct HostRaw {
    T* p = nullptr; size_t cap = 0, n = 0;
    HostRaw() = default; HostRaw(const HostRaw&) = delete; HostRaw& operator=(const HostRaw&) = delete;
    ~HostRaw() { free(p); }
    bool resize(size_t m) {
        if (m > cap) { free(p); cap = m + m / 8 + 16; p = (T*)malloc(cap * sizeof(T)); if (!p) { cap = n = 0; return false; } }
        n = m; return true;
    }
    void clear() { n = 0; }
    T* data() { return p; }
};

struct mdbg_ctx {
    std::recursive_mutex mu;                 // every entry point holds it while it touches the context
    std::mutex err_mu;                       // c->err may be written by callers that only hold a staging slot
    Stage stage[2]; std::mutex stage_mu; std::condition_variable stage_cv;
    mdbg_params P{};
    int dev = 0; hipStream_t stream = nullptr; std::string err; int poisoned = 0;
    u64 scal_seq = 0; bool batchwin_zero = false;      // batchwin_zero: SC_BATCHWIN is known to be 0 on the device
    u64* h_scal = nullptr;                   // pinned, device-visible: the scalars as the last read_scalars() published them
    u64 bound = 0; DevBuf d_t4;              // hash_bound (src/read.rs:183); 4-base tables of the exact evaluation
    // resident sketch store (every read ever ingested since create / reset(0))
    DevBuf mh, mpos, mread, roff; u64 M = 0; u64 mcap = 0; u32 n_slots = 0;
    u64 h_known = 0;                         // staging of the known window count (insert_resident_impl)
    u64 slot_end_m = 0;                      // end (index into mh) of the batch that owns the last slot
    u64 pending_m = 0;                       // minimizers of reserved regions not yet committed (mdbg_sketch_reserve)
    std::vector<Batch> batches; size_t batches_inserted = 0;
    // sketch temporaries
    DevBuf bread, tile_recs, slab, n_valid, n_scan, last_read, tile_base, scan_tmp, gran_sum, tile_flags, scalars, phase_dbg, shards;   // shards: N_SHARD_ARRAYS x CTR_SHARDS u64 (SH_*)
    u32 slab_cap_min = 0;                    // grown when a tile's records did not fit its slab
    // node table
    DevBuf tab, mx; u64 cap = 0;
    // routed records
    DevBuf arena, route_out, route_tmp, route_h, route_f; u64 n_records = 0; bool routed = false;
    // finalize
    DevBuf by_maps;                          // fin_mark's byte maps (2 x 64 bytes per bitmap word)
    DevBuf link_ctr;                         // MDBG_COUNT_LINKS (test hook): one u64, see TableArgs::link_ctr
    DevBuf claim;                            // one byte per resident minimizer index: the window starting there created its key (TableArgs::claim); as large as the store
    bool claims_ok = false;                  // every window in the table was inserted by insert_windows_kernel with the claim map on (set by clear_table / the first table)
    DevBuf bm_first, bm_solid, pre_first, pre_solid, popc_tmp, bt_dev, fin_out, solid_list, fin_order;
    DevBuf bm_local, pre_local, pre_local2;       // partitioned finalize: THIS rank's solid bitmap as it was before the merge over the ranks, and its prefix (the order of the partition's rows)
    HostRaw<u64> h_keys, h_shift_full, h_src_read, h_src_start, h_src_end; HostRaw<u32> h_index, h_seqlen; HostRaw<u16> h_abund, h_shift; HostRaw<u8> h_rev;
    // sketch_only outputs
    std::vector<u64> so_hash, so_pos, so_off;
    // query_batch outputs
    std::vector<u32> q_counts; std::vector<u64> q_off; DevBuf q_dev;
    // synth
    DevBuf syn_bases, syn_off, syn_lens;
    // stats
    u64 n_reads = 0, n_bases = 0, n_windows = 0, n_distinct = 0, n_slow_tiles = 0, n_tiles = 0;
    double ms_sketch = 0, ms_insert = 0, ms_finalize = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev3 = nullptr;      // ev1 (end of the sketch stage) .. ev3: the insertion launched behind the sketch
    // (Rounds 3 - 5 cleared the table on a stream of its own beside the next sketch; the kernel trace showed that it bought nothing — every main-stream kernel ends only when
    // the clear does, profiles/r05_z_clear_overlap.txt — and it cost a launch of its own for the small counters plus two event operations: since round 6 the clear is one
    // launch on the main stream that also zeroes the counters.)
    bool fin_dirty = false;                  // the finalize counters (SC_FIN0..2, SH_FIN_*) may be non-zero: fin_setup zeroes them (else the finalize before left them clean)
    int timing = 2;                          // mdbg_set_timing: 0 no events, 1 around the tile kernel only, 2 also around the stages (ms_sketch / ms_insert / ms_finalize)
    std::vector<u8> bt_sent; const void* bt_sent_at = nullptr;      // the batch table as the device holds it (fin_setup uploads it only when it changed)
    u32 own_world = 1, own_rank = 0;              // replicated-sketch mode: this context inserts only the keys it owns
    int (*before_emit)(void* self, FinArgs& F, u64 n_solid) = nullptr; void* before_emit_self = nullptr;      // mdbg_dist: fetches the positions fin_emit will read from the ranks that hold them
    FinArgs finF{}; u64 fin_words = 0, fin_bits = 0; bool fin_open = false;      // fin_bits: dense ordered indices in use (the batches' minimizers)
    u64 fin_rows_guess = 0;      // fin_rows_guess: rows the next local finalize writes before it knows the count (0: none yet)
    std::vector<u8> bt_host;                 // staging of the batch table (fin_setup)
    EdgeBuffers* eb = nullptr;               // edge construction (edges.hip), created on first use
    DevBuf own_hist;                         // mdbg_owner_counts
    DevBuf own_lists; u64 own_lists_n = 0;   // window lists of the batches this context owns windows of (u32 each), see Batch::list_off
    DevBuf listed_multi; std::vector<ListedBatch> listed_multi_host;      // descriptors of the batches that share one listed-insertion launch
    DevBuf own_thr; u32 thr_world = 0, thr_k = 0; double thr_bound = 0;      // owner_thr()
    DevBuf ol_cnt, ol_off, ol_tot, ol_list, ol_owner;  // mdbg_owner_lists scratch / result
    DevBuf lmer_set; u64 lmer_mask = 0; bool lmer_on = false; u32 lmer_all_ones = 0;      // --lmer-counts: mdbg_set_lmer_filter
    DevBuf w_jstar, w_count, w_ctr, w_start, w_fill, w_occ, w_sorted, w_ath;   // nodes whose u16 abundance wrapped (resolve_wrapped)
    u64 nodes_n = 0; bool nodes_ok = false;  // device node table of the last local finalize is intact
    HostRaw<u32> he_n1, he_n2, he_ov; HostRaw<u8> he_o1, he_o2;           // host copy of the last edge list
    EdgeResult last_edges{}; bool edges_ok = false;                        // device edge list of the last edge call; edges_ok: it belongs to the node table as it stands (unitigs.hip reads both)
    UnitigBuffers* ub = nullptr;             // unitig compaction (unitigs.hip), created on first use
    HostRaw<u64> hu_off, hu_sread, hu_sbegin, hu_dst, hu_length, hu_kc; HostRaw<u32> hu_node, hu_len, hu_n1, hu_n2, hu_ov; HostRaw<u8> hu_ori, hu_rc, hu_circ, hu_o1, hu_o2;   // host copy of the last unitig list
    std::vector<u64> hs_unitigs, hs_nodes;   // per-step removal counts of the last mdbg_graph_simplify
    UnitigResult last_ul{}; bool ulist_ok = false;      // device unitig list of the last unitig / simplify call; ulist_ok: it is current (no edge, finalize, ingest or reset call since)
    ContigBuffers* cb = nullptr;             // contig stitching (contigs.hip), created on first use; its result buffers live until the next contig call
    DevBuf kp_exc_pos, kp_exc_val, kp_cnt;   // keeping an ASCII batch: where the pack kernel appends the (unordered) exceptions, and their count
    HostRaw<u8> hc_bases; HostRaw<u64> hc_off, hc_unitig;      // host copy of the last mdbg_graph_contigs
    double ms_stitch = 0;                    // device time of the last stitch kernel
    std::vector<hipEvent_t> tile_ev; size_t tile_ev_used = 0; double ms_tile = 0; u64 n_tile_launches = 0, n_tile_bases = 0;
};

namespace {

int fail(mdbg_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess) { snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); }   // reported here: do not leave it sticky
    else snprintf(buf, sizeof buf, "%s", what);
    if (c) { std::lock_guard<std::mutex> g_(c->err_mu); c->err = buf; if (code == MDBG_E_DEVICE || code == MDBG_E_ALPHABET || code == MDBG_E_NOMEM) c->poisoned = code; }
    return code;
}
#define MDBG_LOCK(c) std::lock_guard<std::recursive_mutex> lock_((c)->mu)
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), e_ == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, #call, e_); } while (0)
// one column of a copy-out: *host <- the context's host copy `h` of the n elements at `dev` (device memory).  Blocking; `what` names the list in the error.
template <class T> int copy_out(mdbg_ctx* c, HostRaw<T>& h, const T* dev, size_t n, const char* what, const T** host) {
    if (!h.resize(n)) return fail(c, MDBG_E_NOMEM, what);
    if (n) { const hipError_t e = hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost); if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, what, e); }
    *host = h.data();
    return MDBG_OK;
}

u64* scal(mdbg_ctx* c) { return c->scalars.as<u64>(); }
// with_fin: also the two finalize counters (shard arrays 2, 3 -> SC_FIN1, SC_FIN2)
// zero_batchwin: SC_BATCHWIN is reset behind the copy (the next insertion counts its windows into it without a fill in front)
int read_scalars(mdbg_ctx* c, u64* host, bool with_fin = false, bool zero_batchwin = false) {
    if (!c->h_scal) { HIPCHK(c, hipHostMalloc((void**)&c->h_scal, (SC_N + 1) * 8, hipHostMallocMapped)); c->h_scal[SC_N] = 0; }
    const u64 seq = ++c->scal_seq;
    PublishArgs pa{};
    pa.shards[0] = c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS; pa.idx[0] = SC_NDISTINCT; pa.n_arrays = 1;
    pa.zero_mask = 0; pa.zero_arrays = 0;
    if (with_fin) {
        pa.shards[1] = c->shards.as<u64>() + SH_FIN_WRAPPED * CTR_SHARDS; pa.idx[1] = SC_FIN1; pa.shards[2] = c->shards.as<u64>() + SH_FIN_DISTINCT * CTR_SHARDS; pa.idx[2] = SC_FIN2; pa.n_arrays = 3;
        // published, then zeroed: the next finalize finds its counters clean (the host copy below is what the caller works with)
        pa.zero_mask = (1ull << SC_FIN0) | (1ull << SC_FIN1) | (1ull << SC_FIN2); pa.zero_arrays = 0x6u;
    }
    pa.scalars = scal(c); pa.n = SC_N; pa.host = c->h_scal; pa.seq = seq; pa.zero_idx = zero_batchwin ? (u32)SC_BATCHWIN : (u32)SC_N;
    c->batchwin_zero = zero_batchwin;
    launch_publish_scalars(pa, c->stream);
    // the kernel's last store is the sequence number: poll it (a few microseconds after the store) rather than wait for the runtime to see
    // the queue's completion signal; whatever goes wrong on the device ends the wait through the stream's status
    volatile u64* const flag = c->h_scal + SC_N;
    // A short busy poll (what a step of a few milliseconds waits for arrives within it), then polls that give the core away in between (a rank behind a
    // long kernel must not burn a core its reader and packer threads want), then the runtime's own wait.
    bool seen = false;
    const double t0 = now_ms();
    for (u32 spins = 0; !seen; ++spins) {
        seen = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
        if (seen) break;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((spins & 0x3FFu) != 0x3FFu) continue;
        const double waited = now_ms() - t0;
        if (waited > 0.3) std::this_thread::yield();
        if (waited > 20.0) break;
        if ((spins & 0xFFFFu) == 0xFFFFu) { const hipError_t q = hipStreamQuery(c->stream); if (q != hipErrorNotReady) break; }
    }
    if (!seen) HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(host, c->h_scal, SC_N * 8);
    if (with_fin) c->fin_dirty = false;
    return MDBG_OK;
}
int write_scalar(mdbg_ctx* c, int idx, u64 v) {
    HIPCHK(c, hipMemcpyAsync((u64*)c->scalars.p + idx, &v, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MDBG_OK;
}


static void fill_mread_of(mdbg_ctx* c, Batch& b);
// largest hash a selected minimizer can have (0: unknown)
double owner_hash_bound(const mdbg_ctx* c) {
    double b;
    if (c->P.scheme == MDBG_SCHEME_SYNCMERS) { b = c->P.density * ldexp(1.0, 2 * (int)c->P.l); if (b >= 18446744073709551616.0) b = 18446744073709551615.0; }
    else b = (double)c->bound;
    return b >= 1.0 ? b : 0.0;
}
// Parameters of the owner function (table.hip, OwnerSpec) for `world` ranks on the device: thresholds computed when (k, world, hash bound) change — a
// measured bin table (owner_set_table) goes with them and is dropped when they change; null when the hash bound is unknown (then the smallest
// hash is hashed to a rank)
const u64* owner_thr(mdbg_ctx* c, u32 world) {
    if (world <= 1) return nullptr;
    const double b = owner_hash_bound(c);
    if (!(b >= 1.0)) return nullptr;
    if (c->thr_world != world || c->thr_k != c->P.k || c->thr_bound != b) {
        if (c->own_thr.ensure((size_t)OWNER_PARAM_WORDS * 8, 0, c->stream) != hipSuccess) return nullptr;
        launch_owner_thresholds(b, c->P.k, world, c->own_thr.as<u64>(), c->stream);
        c->thr_world = world; c->thr_k = c->P.k; c->thr_bound = b;
    }
    return c->own_thr.as<u64>();
}
// bin = mulhi64(v, multiplier) maps [0, bound] onto OWNER_BINS bins (0: the bound is too small for that, or unknown)
u64 owner_bin_mul(const mdbg_ctx* c) {
    const double b = owner_hash_bound(c);
    if (!(b >= (double)OWNER_BINS * 4.0)) return 0;
    u64 bi = b >= 18446744073709549568.0 ? ~0ull : (u64)b;
    const unsigned __int128 q = ((unsigned __int128)OWNER_BINS << 64) / ((unsigned __int128)bi + 1);
    return q > (unsigned __int128)~0ull ? 0 : (u64)q;
}
// window minima of one resident batch counted per bin into d_hist[OWNER_BINS] (added to; stream-ordered)
int owner_hist_batch(mdbg_ctx* c, size_t which, u64* d_hist) {
    const u64 mul = owner_bin_mul(c);
    if (!mul || c->batches.empty()) return MDBG_OK;
    Batch& b = which == ~(size_t)0 ? c->batches.back() : c->batches[which];
    fill_mread_of(c, b);
    launch_owner_bins(c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, mul, d_hist, c->stream);
    return MDBG_OK;
}
// the measured assignment: tab[OWNER_BINS] = owner of every bin (host memory), for `world` ranks
int owner_set_table(mdbg_ctx* c, u32 world, const u8* tab) {
    const u64 mul = owner_bin_mul(c);
    if (!mul || !owner_thr(c, world)) return MDBG_OK;                 // no table for these parameters: the thresholds stay
    HIPCHK(c, hipMemcpyAsync(c->own_thr.as<u64>() + OWNER_TAB_AT, tab, OWNER_BINS, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->own_thr.as<u64>(), &mul, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                       // (tab / mul are the caller's and a local)
    return MDBG_OK;
}
TableArgs table_args(mdbg_ctx* c) {
    TableArgs T;
    T.tab = c->tab.as<Slot>(); T.cap = c->cap; T.mx = c->mx.as<u64>(); T.A = cascade_of(c->P.min_abundance);
    T.n_distinct = c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS;
    T.ks.mh = c->mh.as<u64>(); T.ks.arena = c->arena.as<u64>(); T.ks.k = c->P.k;
    T.own_world = c->own_world; T.own_rank = c->own_rank; T.own_thr = owner_thr(c, c->own_world);
    T.probe_err = (u32*)(scal(c) + SC_PROBEERR); T.own_inserted = c->shards.as<u64>() + SH_OWNINS * CTR_SHARDS;
    T.claim = (!c->routed && c->claims_ok) ? c->claim.as<u8>() : nullptr;      // (partitioned tables too since round 6: every insertion kernel of resident windows writes its claims)
    static const bool no_chain = getenv("MDBG_NO_CHAIN") != nullptr;      // (A/B switch and test hook: every fingerprint hit is confirmed by the full comparison)
    T.no_chain = no_chain ? 1u : 0u;
    static const bool weak_fp = getenv("MDBG_WEAK_FP") != nullptr;        // (test hook: a two-bit fingerprint; the table stays exact, the comparisons and the walks behind them get exercised)
    T.fp_mask = weak_fp ? 0x3ull : 0x3FFFFFFFull;
    static const bool count_links = getenv("MDBG_COUNT_LINKS") != nullptr;
    T.link_ctr = nullptr;
    if (count_links) {
        if (!c->link_ctr.p && c->link_ctr.ensure(8, 0, c->stream) == hipSuccess) (void)hipMemsetAsync(c->link_ctr.p, 0, 8, c->stream);
        T.link_ctr = (unsigned long long*)c->link_ctr.p;
    }
    return T;
}

// slots for n keys at load factor <= 2/3 (linear probing; the capacity need not be a power of two, see home_slot)
u64 slots_for(u64 n) { return n + n / 2 + 1024; }

// make room for `incoming` more occurrences (each possibly a new key)
int table_reserve(mdbg_ctx* c, u64 incoming) {
    u64 need = slots_for(c->n_distinct + incoming);
    const u32 A = cascade_of(c->P.min_abundance);
    if (c->cap == 0) {
        u64 want = need;
        if (c->P.table_capacity_hint) want = std::max(want, slots_for(c->P.table_capacity_hint));
        HIPCHK(c, c->tab.ensure(want * sizeof(Slot), 0, c->stream));
        if (A > 2) HIPCHK(c, c->mx.ensure(want * (A - 2) * 8, 0, c->stream));
        c->cap = want;
        launch_clear_table(c->tab.as<Slot>(), c->cap, c->mx.as<u64>(), A > 2 ? c->cap * (A - 2) : 0, c->stream);
        c->claims_ok = !c->routed && c->claim.p != nullptr;      // an empty table: from here on every insertion writes its claims
        return MDBG_OK;
    }
    if (need <= c->cap) return MDBG_OK;
    // grow (at least doubling, so that batch-wise ingestion rehashes O(log) times) and rehash
    need = std::max(need, 2 * c->cap);
    DevBuf ntab, nmx;
    HIPCHK(c, ntab.ensure(need * sizeof(Slot), 0, c->stream));
    if (A > 2) HIPCHK(c, nmx.ensure(need * (A - 2) * 8, 0, c->stream));
    launch_clear_table(ntab.as<Slot>(), need, nmx.as<u64>(), A > 2 ? need * (A - 2) : 0, c->stream);
    TableArgs T = table_args(c);
    T.tab = ntab.as<Slot>(); T.cap = need; T.mx = nmx.as<u64>();
    launch_rehash(c->tab.as<Slot>(), c->cap, c->mx.as<u64>(), T, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(c->tab.p, ntab.p); std::swap(c->tab.cap, ntab.cap);
    std::swap(c->mx.p, nmx.p); std::swap(c->mx.cap, nmx.cap);
    c->cap = need;
    return MDBG_OK;
}

int clear_table(mdbg_ctx* c) {
    c->nodes_ok = false; c->ulist_ok = false;
    // the key counter's shards, SC_NDISTINCT + SC_NWINDOWS, SC_IMPORTERR, SC_PROBEERR: zeroed by the launch that clears the table (stream-ordered, no host sync) — or by
    // a launch of their own when there is no table yet
    ZeroList z{};
    z.p[0] = c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS; z.n[0] = CTR_SHARDS; z.p[1] = scal(c) + SC_NDISTINCT; z.n[1] = 2;
    z.p[2] = scal(c) + SC_IMPORTERR; z.n[2] = 1; z.p[3] = scal(c) + SC_PROBEERR; z.n[3] = 1;
    if (c->cap) launch_clear_table(c->tab.as<Slot>(), c->cap, c->mx.as<u64>(), cascade_of(c->P.min_abundance) > 2 ? c->cap * (cascade_of(c->P.min_abundance) - 2) : 0, c->stream, &z);
    else launch_zero_regions(z, c->stream);
    c->n_distinct = 0; c->n_windows = 0; c->batches_inserted = 0; c->n_records = 0; c->routed = false;
    c->claims_ok = c->claim.p != nullptr;
    return MDBG_OK;
}

// an event costs ~4 microseconds of stream time (scratch/ubench/event_cost.hip: a marker packet with a timestamp), six of them per ingested batch and two per finalize
// were 1.7 % of a configs[2] step: mdbg_set_timing chooses which are recorded
#define STAGE_EVENT(c, ev, s) do { if ((c)->timing >= 2) HIPCHK((c), hipEventRecord((ev), (s))); } while (0)
hipEvent_t next_tile_event(mdbg_ctx* c) {
    if (c->timing < 1) return nullptr;
    if (c->tile_ev_used == c->tile_ev.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; c->tile_ev.push_back(e); }
    return c->tile_ev[c->tile_ev_used++];
}
void collect_tile_events(mdbg_ctx* c) {      // after a stream sync
    for (size_t i = 0; i + 1 < c->tile_ev_used; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->tile_ev[i], c->tile_ev[i + 1]) == hipSuccess) c->ms_tile += ms;
        else (void)hipGetLastError();      // never leave a sticky error behind for the next user of the HIP runtime (torch)
    }
    c->tile_ev_used = 0;
}
float ev_ms(mdbg_ctx* c) {
    float ms = 0;
    if (c->timing < 2) return 0.0f;
    (void)hipEventSynchronize(c->ev1);       // (callers have waited for the stream already; an event the runtime has not retired yet would read as 0)
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
    return ms;
}

int check_params(const mdbg_params* p) {
    if (!p) return MDBG_E_PARAM;
    if (p->k < 2 || p->k > 4096) return MDBG_E_PARAM;
    if (p->l < 2 || p->l > MDBG_MAX_L) return MDBG_E_PARAM;
    if (p->min_abundance < 1 || p->min_abundance > MDBG_MAX_MINABUND) return MDBG_E_PARAM;      // DbgAbundance is a u16 in the reference
    if (!(p->density == p->density)) return MDBG_E_PARAM;
    if (p->scheme > MDBG_SCHEME_SYNCMERS) return MDBG_E_PARAM;
    if (p->scheme == MDBG_SCHEME_SYNCMERS && (p->l > 31 || p->syncmer_s > 16 || p->syncmer_s > p->l || p->l - p->syncmer_s + 1 > 32)) return MDBG_E_PARAM;
    return MDBG_OK;
}

// Grow the resident sketch store to at least want_m minimizers.  Refused while reserved regions await their data: the
// caller's receive (RCCL) would land in freed memory.
int store_ensure(mdbg_ctx* c, u64 want_m) {
    if (want_m <= c->mcap) return MDBG_OK;
    if (c->pending_m) return fail(c, MDBG_E_STATE, "the sketch store would have to move while reserved regions are pending (commit them, or size the store up front with mdbg_store_reserve)");
    hipStream_t s = c->stream;
    HIPCHK(c, c->mh.ensure(want_m * 8, c->M * 8, s));
    HIPCHK(c, c->mpos.ensure(want_m * 4, c->M * 4, s));
    HIPCHK(c, c->mread.ensure(want_m * 4, c->M * 4, s));
    HIPCHK(c, c->claim.ensure(want_m + 128, c->M, s));
    c->mcap = want_m;
    return MDBG_OK;
}
// First slot of a new batch whose minimizers start at m0.  Batches that are adjacent in the store share the boundary
// entry of roff; when there is a gap (a reserved region in between) one unused slot keeps the previous batch's end intact.
int next_slot0(mdbg_ctx* c, u64 m0, u64 n_reads, u32* slot0) {
    if (!c->batches.empty() && c->slot_end_m != m0) c->n_slots += 1;
    if ((u64)c->n_slots + n_reads >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many reads");
    *slot0 = c->n_slots;
    HIPCHK(c, c->roff.ensure(((u64)c->n_slots + n_reads + 2) * 8, ((u64)c->n_slots + 1) * 8, c->stream));
    return MDBG_OK;
}

// the sketch stage over a device-resident batch (ASCII or 2-bit planes); appends to the resident store and records a Batch
struct SketchInput {
    u32 fmt = FMT_ASCII;
    const u8* d_bases = nullptr;             // FMT_ASCII
    const uint2* d_planes = nullptr;         // FMT_PLANES: ceil(n_bases / 32) pairs
    const u64* d_exc_pos = nullptr; const u8* d_exc_val = nullptr; u64 n_exc = 0;   // FMT_PLANES: bytes outside ACGT, sorted by position
};
int insert_resident_impl(mdbg_ctx* c, bool allow_pending = false);

// MDBG_FLAG_KEEP_READS: a packed device copy of the batch that has just been sketched (the caller's buffers are still valid; the staging buffers of the
// host entry points are reused by the next batch, so nothing is borrowed).  ASCII is packed by the kernel behind mdbg_pack_device; its exception list
// comes back unordered and is sorted on the device (rocPRIM), so the only host round trip is the 8-byte count that sizes the side-list — and that one
// only exists on a context that keeps reads.  Packed input is copied device to device.  Words and offsets are kept from base 0 of the batch, so a device
// ASCII batch with offsets[0] > 0 keeps its offsets as they are (relative to the kept words).
int keep_batch(mdbg_ctx* c, const SketchInput& in, const u64* d_offsets, u64 n_reads, u64 n_bases, std::shared_ptr<KeptReads>& out) {
    hipStream_t s = c->stream;
    std::shared_ptr<KeptReads> k = std::make_shared<KeptReads>();
    k->n_reads = n_reads; k->n_bases = n_bases; k->n_words = (n_bases + 31) / 32;
    HIPCHK(c, mdbg_block_alloc(&k->blk, k->n_words * 8 + (n_reads + 1) * 8, &k->cap));
    HIPCHK(c, hipMemcpyAsync(k->offsets(), d_offsets, (n_reads + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (in.fmt == FMT_PLANES) {
        if (k->n_words) HIPCHK(c, hipMemcpyAsync(k->planes(), in.d_planes, k->n_words * 8, hipMemcpyDeviceToDevice, s));
        k->n_exc = in.n_exc;
        if (k->n_exc) {
            HIPCHK(c, mdbg_block_alloc(&k->xblk, k->n_exc * 9, &k->xcap));
            HIPCHK(c, hipMemcpyAsync(k->exc_pos(), in.d_exc_pos, k->n_exc * 8, hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipMemcpyAsync(k->exc_val(), in.d_exc_val, k->n_exc, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK(c, hipStreamSynchronize(s));      // the source buffers are the caller's (or a staging slot's) once the ingest call returns
    } else if (k->n_words) {
        HIPCHK(c, c->kp_cnt.ensure(8, 0, s));
        u64 cap = std::max<u64>(c->kp_exc_pos.cap / 8, 4096), n = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {      // a second time only when the side-list was too small for what the first pass counted
            HIPCHK(c, c->kp_exc_pos.ensure(cap * 8, 0, s)); HIPCHK(c, c->kp_exc_val.ensure(cap, 0, s));
            HIPCHK(c, hipMemsetAsync(c->kp_cnt.p, 0, 8, s));
            launch_pack_planes(in.d_bases, n_bases, k->planes(), c->kp_exc_pos.as<u64>(), c->kp_exc_val.as<u8>(), cap, (unsigned long long*)c->kp_cnt.p, s);
            HIPCHK(c, hipMemcpyAsync(&n, c->kp_cnt.p, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (n <= cap) break;
            cap = n;
        }
        if (n > cap) return fail(c, MDBG_E_DEVICE, "the exception count of a kept batch changed between two passes");
        k->n_exc = n;
        if (n) {
            HIPCHK(c, mdbg_block_alloc(&k->xblk, n * 9, &k->xcap));
            if (!c->cb) c->cb = contig_buffers_create();
            HIPCHK(c, sort_exceptions(c->cb, c->kp_exc_pos.as<u64>(), c->kp_exc_val.as<u8>(), k->exc_pos(), k->exc_val(), n, s));
        }
    } else HIPCHK(c, hipStreamSynchronize(s));
    out = std::move(k);
    return MDBG_OK;
}
// then_insert: the caller inserts the batch's windows right away.  When nothing stands in the way (a table exists, one launch, no filter, nothing
// else pending) the window count, the capacity check and the insertion are launched BEHIND the sketch before the host has looked at it — one host
// round trip per batch instead of two; the device-side check also stops the insertion when the sketch has to be repeated.  *inserted tells the caller.
int sketch_device_impl(mdbg_ctx* c, const SketchInput& in, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 first_ordinal, bool then_insert = false, bool* inserted = nullptr) {
    if (inserted) *inserted = false;
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (n_reads == 0) return MDBG_OK;
    if (in.fmt == FMT_ASCII && !in.d_bases && n_bases) return fail(c, MDBG_E_PARAM, "null bases");
    if (in.fmt == FMT_PLANES && !in.d_planes && n_bases) return fail(c, MDBG_E_PARAM, "null packed words");
    if (!d_offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if ((((uintptr_t)in.d_bases) | ((uintptr_t)in.d_planes)) & 15) return fail(c, MDBG_E_PARAM, "device bases pointer must be 16-byte aligned");
    if (in.n_exc && (!in.d_exc_pos || !in.d_exc_val)) return fail(c, MDBG_E_PARAM, "null exception list");
    if (in.n_exc >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many exceptions");
    if (n_reads >= 0xFFFFFFF0ull || (u64)c->n_slots + n_reads >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many reads");
    if (first_ordinal + n_reads >= (1ull << (64 - WIN_BITS))) return fail(c, MDBG_E_CAPACITY, "read ordinal too large");
    hipStream_t s = c->stream;
    const bool sync = c->P.scheme == MDBG_SCHEME_SYNCMERS;
    const u64 tile_bases = TILE_STRIDE;
    const u64 n_tiles_total = (n_bases + tile_bases - 1) / tile_bases;
    if (n_tiles_total >= 0x7FFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "batch too large for one call");
    u32 slot0 = 0;
    { int e = next_slot0(c, c->M, n_reads, &slot0); if (e) return e; }
    double dens2 = 2.0 * c->P.density; if (dens2 > 1.0) dens2 = 1.0; if (dens2 < 0) dens2 = 0;
    // records per tile slab: expectation for i.i.d. hashes + 25 % + 6 sigma; a tile that still overflows makes the batch run again
    // with slabs sized from the largest count seen (and the context remembers that size)
    u32 slab_cap = 0, gather_tiles = 1;
    {
        // syncmers: about one l-mer in l-s+1 has its smallest s-mer in the middle, of which a fraction `density` survives
        const double per_base = sync ? std::min(1.0, std::max(0.0, c->P.density)) / (c->P.syncmer_s ? std::max(1.0, (double)(c->P.l - c->P.syncmer_s + 1) / 2.0) : 1.0) : dens2;
        const double e = (double)tile_bases * per_base; double v = e * 1.25 + 6.0 * sqrt(e) + 32.0; if (v > (double)tile_bases) v = (double)tile_bases; slab_cap = ((u32)v + 7u) & ~7u;
        // small tiles: one gather wave takes several (about 256 expected records)
        if (e < 128.0) gather_tiles = (u32)std::max(1.0, std::min(16.0, 256.0 / std::max(e, 1.0)));
    }
    if (slab_cap < c->slab_cap_min) slab_cap = c->slab_cap_min;
    // test hooks: MDBG_SLAB_CAP0 = slab size of a context's FIRST attempt (small: the tiles overflow and the batch runs again with slabs sized from what was seen),
    // MDBG_SLAB_BUDGET_MB = bytes of slabs per launch (small: several launches per batch)
    static const u32 cap0_hook = getenv("MDBG_SLAB_CAP0") ? (u32)atoi(getenv("MDBG_SLAB_CAP0")) : 0u;
    static const u64 budget_hook = getenv("MDBG_SLAB_BUDGET_MB") ? (u64)atoll(getenv("MDBG_SLAB_BUDGET_MB")) << 20 : 0ull;
    if (cap0_hook && !c->slab_cap_min) slab_cap = std::max<u32>(8u, cap0_hook & ~7u);
    if (slab_cap > (u32)tile_bases) slab_cap = (u32)tile_bases;
    if (n_tiles_total) {
        HIPCHK(c, c->bread.ensure((n_tiles_total + 2) * 4, 0, s));
        HIPCHK(c, c->tile_recs.ensure(n_tiles_total * sizeof(TileRec), 0, s));
        HIPCHK(c, c->n_valid.ensure(n_tiles_total * 4, 0, s));
        HIPCHK(c, c->n_scan.ensure(n_tiles_total * 4, 0, s));
        HIPCHK(c, c->last_read.ensure(n_tiles_total * 4, 0, s));
        if (in.n_exc) HIPCHK(c, c->tile_flags.ensure(n_tiles_total, 0, s));
    }
    u64 want = c->M + (u64)((double)n_bases * dens2 * 1.15) + 65536;
    const bool phase_dbg = getenv("MDBG_PHASE_TIMING") != nullptr;      // per-phase cycle stamps of the tile kernel (diagnostic)
    for (int attempt = 0; attempt < 4; ++attempt) {
        { int e = store_ensure(c, want); if (e) return e; }
        // tiles per launch: the slabs of one launch stay under SLAB_BUDGET bytes (one launch for every BASELINE configuration; dense settings
        // run in several, one after the other).  Measured and dropped this round: cutting a batch into 2-4 parts whose scan + gather run on
        // a second stream under the next part's tile kernel — the copy slows the tile kernel down by as much as it hides (profiles/r03_notes.md).
        const u64 chunk = std::max<u64>(1, std::min<u64>(n_tiles_total ? n_tiles_total : 1, (budget_hook ? budget_hook : SLAB_BUDGET) / ((u64)slab_cap * sizeof(Rec))));
        std::vector<u64> part_end;                  // exclusive end tile of every launch
        for (u64 t0 = 0; t0 < n_tiles_total; t0 += chunk) part_end.push_back(std::min<u64>(n_tiles_total, t0 + chunk));
        u64 max_part = 0; { u64 t0 = 0; for (u64 e : part_end) { max_part = std::max(max_part, e - t0); t0 = e; } }
        if (n_tiles_total) {
            HIPCHK(c, c->slab.ensure((size_t)chunk * slab_cap * sizeof(Rec), 0, s));
            HIPCHK(c, c->tile_base.ensure((size_t)max_part * 8, 0, s));
            HIPCHK(c, c->scan_tmp.ensure(((size_t)max_part / 1024 + 2) * 8, 0, s));
        }
        u64 init[1] = {c->M};
        STAGE_EVENT(c, c->ev0, s);
        // SC_CARRY = M, the error / slow-tile / overflow scalars = 0: by the kernel that prepares the tile records (or a launch of their own)
        SketchInit init0{};
        init0.zero[0] = scal(c) + SC_ERRFLAG; init0.zero[1] = scal(c) + SC_SLOWTOTAL; init0.zero[2] = scal(c) + SC_OVERMAX; init0.set_p = scal(c) + SC_CARRY; init0.set_v = c->M;
        // the insertion can ride behind this sketch when its grid can be sized without the count: the store's free room is the bound, and it must not be
        // much more than the batch is expected to fill (a store sized for many batches would launch mostly idle workgroups)
        const bool fused = then_insert && inserted && n_tiles_total && part_end.size() == 1 && !phase_dbg && c->cap && c->own_world <= 1 && !c->lmer_on && !c->routed && !c->pending_m &&
                           c->batches_inserted == c->batches.size() && c->mcap > c->M && c->mcap - c->M <= 2 * (want - c->M) + (1u << 20) &&
                           want - c->M <= (48ull << 20);          // (larger rounds are inserted in slices, insert_resident_impl)
        if (fused) init0.zero[3] = scal(c) + SC_BATCHWIN;
        if (!n_tiles_total) {
            ZeroList z{};
            z.p[0] = init0.zero[0]; z.n[0] = 1; z.p[1] = init0.zero[1]; z.n[1] = 1; z.p[2] = init0.zero[2]; z.n[2] = 1; z.set_p = init0.set_p; z.set_v = init0.set_v;
            launch_zero_regions(z, s);
            // a batch of empty reads only: no tile, so no gather writes the reads' offsets — every one of them starts and ends at M.  (They were left as the
            // allocation came: zero from a fresh hipMalloc, which is what M is for a first batch; found by the fuzz in a process that had freed memory before.)
            launch_fill_u64(c->roff.as<u64>() + slot0, n_reads + 1, c->M, s);
        }
        SketchArgs A{};
        A.bases = in.d_bases; A.planes = in.d_planes; A.fmt = in.fmt; A.n_bases = n_bases; A.offsets = d_offsets; A.n_reads = (u32)n_reads;
        A.exc_pos = in.d_exc_pos; A.exc_val = in.d_exc_val; A.n_exc = (u32)in.n_exc;
        A.l = c->P.l; A.hpc = c->P.reads_already_hpc == 0 ? 1u : 0u;
        if (n_tiles_total) {
            A.bread = c->bread.as<u32>(); A.recs = c->tile_recs.as<TileRec>(); A.n_tiles = (u32)n_tiles_total;
            A.slab = c->slab.as<Rec>(); A.slab_cap = slab_cap; A.n_valid = c->n_valid.as<u32>(); A.n_scan = c->n_scan.as<u32>(); A.last_read = c->last_read.as<u32>(); A.over_max = (u32*)(scal(c) + SC_OVERMAX);
            A.t4 = c->d_t4.as<u64>();
            A.tile_flags = in.n_exc ? c->tile_flags.as<u8>() : nullptr;
            A.err_flag = (u32*)(scal(c) + SC_ERRFLAG); A.slow_total = (unsigned long long*)(scal(c) + SC_SLOWTOTAL);
            A.read_base = slot0; A.bound = c->bound; A.btop = (u32)(c->bound >> (64 - BS_B)); A.force_slow = ((c->P.flags & 1u) || c->P.l > (u32)BS_MAX_L) ? 1u : 0u;      // l > 32: the generic exact walker handles any l
            A.dbg = nullptr;
            { const char* sp = getenv("MDBG_STOP_PHASE"); A.stop_phase = sp ? (u32)atoi(sp) : 0u; }
            if (phase_dbg) { HIPCHK(c, c->phase_dbg.ensure((size_t)n_tiles_total * 128, 0, s)); HIPCHK(c, hipMemsetAsync(c->phase_dbg.p, 0, (size_t)n_tiles_total * 128, s)); A.dbg = c->phase_dbg.as<u64>(); }
            // the first level of the gather's scan is accumulated by the tiles themselves (SketchArgs::block_sum; zeroed by the kernel that prepares the tile records)
            const u32 n_gran = (u32)((max_part + SCAN_GRAN - 1) / SCAN_GRAN);
            HIPCHK(c, c->gran_sum.ensure((size_t)n_gran * 8 + 64, 0, s));
            A.block_sum = (unsigned long long*)c->gran_sum.as<u64>();
            init0.zero_arr = c->gran_sum.as<u64>(); init0.zero_arr_n = n_gran;
            launch_bread(d_offsets, (u32)n_reads, n_bases, A.n_tiles, c->bread.as<u32>(), c->tile_recs.as<TileRec>(), init0, s);
            if (in.n_exc) {
                HIPCHK(c, hipMemsetAsync(c->tile_flags.p, 0, n_tiles_total, s));
                launch_tile_flags(in.d_exc_pos, (u32)in.n_exc, A.n_tiles, c->tile_flags.as<u8>(), s);
            }
            if (sync) {
                A.scheme = 1; A.s = c->P.syncmer_s; A.btop = 0;
                const double v = c->P.density * (double)(1ull << (2 * c->P.l));           // src/read.rs:218, saturating cast
                A.bound = !(v > 0.0) ? 0 : (v >= 18446744073709551616.0 ? ~0ull : (u64)v);
                A.force_slow = ((c->P.flags & 1u) || c->P.syncmer_s > 13) ? 1u : 0u;      // the register window packs hash << 5 | age: s <= 13; longer s-mers take the generic machine
            }
            u64 t0 = 0;
            for (size_t pi = 0; pi < part_end.size(); ++pi) {
                const u32 nt = (u32)(part_end[pi] - t0);
                Rec* const part_slab = c->slab.as<Rec>();
                A.tile0 = (u32)t0; A.slab = part_slab;
                if (pi) HIPCHK(c, hipMemsetAsync(c->gran_sum.p, 0, (size_t)n_gran * 8, s));      // (several launches per batch — dense settings —: the next launch's sums start from zero)
                { hipEvent_t tb = next_tile_event(c), te = next_tile_event(c); launch_sketch(A, nt, s, tb, te); }
                GatherArgs G{};
                G.tile0 = (u32)t0; G.n = nt; G.slab = part_slab; G.slab_cap = slab_cap; G.n_valid = A.n_valid; G.n_scan = A.n_scan; G.last_read = A.last_read;
                G.out_hash = c->mh.as<u64>(); G.out_pos = c->mpos.as<u32>(); G.out_read = c->mread.as<u32>(); G.out_cap = c->mcap;
                G.m0 = c->M; G.slot0 = slot0; G.n_reads = (u32)n_reads; G.off = c->roff.as<u64>(); G.last_launch = pi + 1 == part_end.size() ? 1u : 0u;
                G.tiles_per_wave = gather_tiles;
                launch_gather(G, c->scan_tmp.as<u64>(), c->tile_base.as<u64>(), scal(c) + SC_CARRY, s, c->gran_sum.as<u64>());
                c->n_tile_launches += 1;
                t0 = part_end[pi];
            }
            c->n_tile_bases += n_bases;
            if (phase_dbg) {
                std::vector<u64> h((size_t)A.n_tiles * 16);
                (void)hipStreamSynchronize(s);
                (void)hipMemcpy(h.data(), A.dbg, h.size() * 8, hipMemcpyDeviceToHost);
                double ph[7] = {0, 0, 0, 0, 0, 0, 0}, nc = 0, nv = 0; u64 nfast = 0;
                for (u32 t = 0; t < A.n_tiles; ++t) {
                    const u64* q = &h[(size_t)t * 16];
                    if (!q[7]) continue;               // generic path: no stamps
                    ++nfast;
                    ph[0] += (double)(q[1] - q[0]); ph[1] += (double)(q[2] - q[1]); ph[2] += (double)(q[3] - q[2]); ph[3] += (double)(q[4] - q[3]);
                    ph[4] += (double)(q[5] - q[4]); ph[5] += (double)(q[7] - q[5]);
                    nc += (double)q[9]; nv += (double)q[10];
                }
                const double n = nfast ? (double)nfast : 1.0;
                fprintf(stderr, "[mdbg phase timing] tiles=%u fast=%llu avg cycles: load=%.0f compact=%.0f hash=%.0f exact=%.0f rank=%.0f write=%.0f ; candidates=%.1f valid=%.1f slab_cap=%u\n",
                        A.n_tiles, (unsigned long long)nfast, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n, ph[4] / n, ph[5] / n, nc / n, nv / n, slab_cap);
            }
        }
        STAGE_EVENT(c, c->ev1, s);                                         // end of the sketch stage = start of the insertion when it rides behind
        u32* const ins_flags = (u32*)(scal(c) + SC_CAPERR);                // [0] window index overflow, [1] table too small / sketch to be repeated
        if (fused) {
            // the window count and the capacity check in ONE launch (count_reserve_kernel)
            launch_count_reserve(c->roff.as<u64>(), slot0, (u32)n_reads, c->P.k, scal(c) + SC_BATCHWIN, (u32*)(scal(c) + SC_DONE), c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS, scal(c) + SC_NDISTINCT,
                                 c->cap, ins_flags + 1, scal(c) + SC_CARRY, c->mcap, (const u32*)(scal(c) + SC_OVERMAX), s);
            if (!c->ev3) HIPCHK(c, hipEventCreate(&c->ev3));
            launch_insert_windows(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), c->M, c->mcap, slot0, first_ordinal, scal(c) + SC_NWINDOWS, ins_flags, s, scal(c) + SC_CARRY);
            STAGE_EVENT(c, c->ev3, s);
        }
        u64 sc[SC_N];
        int e = read_scalars(c, sc, false, true); if (e) return e;
        c->ms_sketch += ev_ms(c);
        collect_tile_events(c);
        u64 m_new = sc[SC_CARRY];
        const u32 over = (u32)sc[SC_OVERMAX];
        if (over || m_new > c->mcap) {           // a slab or the store was too small: size them from what was seen and run the batch again
            if (over) { slab_cap = std::min<u32>((u32)tile_bases, (over + over / 8 + 15u) & ~7u); c->slab_cap_min = slab_cap; }
            if (m_new > c->mcap) want = m_new + 65536;
            c->n_tile_launches -= part_end.size(); c->n_tile_bases -= n_tiles_total ? n_bases : 0;
            continue;
        }
        if (m_new >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers resident on one device");
        if ((u32)sc[SC_ERRFLAG]) {
            // a byte outside ACGTN was seen somewhere: apply the reference's exact rule (alphabet_rule_kernel)
            u64 which = ~0ull;
            HIPCHK(c, hipMemcpyAsync(scal(c) + SC_SLOWTOTAL, &which, 8, hipMemcpyHostToDevice, s));      // scratch use of a scalar that was read already
            launch_alphabet_rule(A, (unsigned long long*)(scal(c) + SC_SLOWTOTAL), s);
            HIPCHK(c, hipMemcpyAsync(&which, scal(c) + SC_SLOWTOTAL, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (which != ~0ull) {
                char buf[160]; snprintf(buf, sizeof buf, "Non-ACGTN nucleotide in read %llu of the batch (ordinal %llu)", (unsigned long long)which, (unsigned long long)(first_ordinal + which));
                return fail(c, MDBG_E_ALPHABET, buf);
            }
        }
        const u64 slow_total = sc[SC_SLOWTOTAL];      // (the scalar is scratch from here on)
        if (c->lmer_on && m_new > c->M) {
            // --lmer-counts: of the minimizers that passed the threshold keep those whose l-mer is in the set (read.rs:200-205); the
            // survivors go through slabs of 256 and the sketch's gather back to the same place in the store
            const u32 nb = lmer_filter_blocks(m_new - c->M);
            HIPCHK(c, c->slab.ensure((size_t)nb * 256 * sizeof(Rec), 0, s));
            HIPCHK(c, c->n_valid.ensure((size_t)nb * 4, 0, s)); HIPCHK(c, c->tile_base.ensure((size_t)nb * 8, 0, s)); HIPCHK(c, c->scan_tmp.ensure(((size_t)nb / 1024 + 2) * 8, 0, s));
            LmerFilterArgs L{};
            L.set = c->lmer_set.as<u64>(); L.set_mask = c->lmer_mask; L.has_all_ones = c->lmer_all_ones;
            L.mh = c->mh.as<u64>(); L.mpos = c->mpos.as<u32>(); L.mread = c->mread.as<u32>(); L.m0 = c->M; L.m1 = m_new;
            L.offsets = d_offsets; L.slot0 = slot0; L.l = c->P.l; L.hpc = c->P.reads_already_hpc == 0 ? 1u : 0u;
            L.slab = c->slab.as<Rec>(); L.n_valid = c->n_valid.as<u32>();
            launch_lmer_filter(L, in.fmt, in.d_bases, in.d_planes, in.d_exc_pos, in.d_exc_val, (u32)in.n_exc, s);
            HIPCHK(c, hipMemcpyAsync(scal(c) + SC_CARRY, init, 8, hipMemcpyHostToDevice, s));
            GatherArgs G{};
            G.tile0 = 0; G.n = nb; G.slab = L.slab; G.slab_cap = 256; G.n_valid = L.n_valid;
            G.out_hash = c->mh.as<u64>(); G.out_pos = c->mpos.as<u32>(); G.out_read = c->mread.as<u32>(); G.out_cap = c->mcap;
            G.m0 = c->M; G.slot0 = slot0; G.n_reads = (u32)n_reads; G.off = c->roff.as<u64>(); G.last_launch = 1; G.tiles_per_wave = 1;      // the offsets of the filtered set replace the first pass's
            launch_gather(G, c->scan_tmp.as<u64>(), c->tile_base.as<u64>(), scal(c) + SC_CARRY, s);
            int e2 = read_scalars(c, sc); if (e2) return e2;
            m_new = sc[SC_CARRY];
        }
        Batch b; b.first_ordinal = first_ordinal; b.n_reads = (u32)n_reads; b.slot0 = slot0; b.m0 = c->M; b.m1 = m_new; b.n_bases = n_bases;
        c->ulist_ok = false;                     // an ingest ends the current unitig list (mdbg_graph_contigs)
        if (c->P.flags & MDBG_FLAG_KEEP_READS) { int ke = keep_batch(c, in, d_offsets, n_reads, n_bases, b.kept); if (ke) return ke; }
        c->batches.push_back(b);
        c->M = m_new; c->n_slots = slot0 + (u32)n_reads; c->slot_end_m = m_new;
        c->n_reads += n_reads; c->n_bases += n_bases; c->n_tiles += n_tiles_total; c->n_slow_tiles += slow_total;
        if (fused) {             // the table side of the same round trip (the tail of insert_resident_impl)
            c->nodes_ok = false;
            if (sc[SC_CAPERR] >> 32) return MDBG_OK;   // the sketch was fine, so the table was too small: nothing was inserted; the caller inserts the plain way (*inserted stays false)
            c->batches_inserted = c->batches.size();
            *inserted = true;
            if ((u32)sc[SC_PROBEERR]) return fail(c, MDBG_E_PARAM, "the table filled up during insertion");
            float ms = 0;
            if (c->timing >= 2) { if (hipEventElapsedTime(&ms, c->ev1, c->ev3) == hipSuccess) c->ms_insert += ms; else (void)hipGetLastError(); }
            c->n_windows += sc[SC_BATCHWIN];
            c->n_distinct = sc[SC_NDISTINCT];
            if (sc[SC_IMPORTERR]) return fail(c, MDBG_E_PARAM, "read offsets of an imported sketch are not consistent with its size");
            if ((u32)sc[SC_CAPERR]) return fail(c, MDBG_E_CAPACITY, "a read has more than 2^26 minimizers");
        }
        return MDBG_OK;
    }
    return fail(c, MDBG_E_CAPACITY, "minimizer store could not be sized");
}
int sketch_device_impl(mdbg_ctx* c, const u8* d_bases, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 first_ordinal, bool then_insert = false, bool* inserted = nullptr) {
    SketchInput in; in.fmt = FMT_ASCII; in.d_bases = d_bases;
    return sketch_device_impl(c, in, d_offsets, n_reads, n_bases, first_ordinal, then_insert, inserted);
}

// The minimizer -> read map of a batch that was imported with a window list is only written where the table needs it (the
// representatives, insert_listed_*); every other consumer asks for the whole map first.
static void fill_mread_of(mdbg_ctx* c, Batch& b) {
    if (b.mread_ok) return;
    launch_fill_mread(c->roff.as<u64>(), b.slot0, b.n_reads, c->mread.as<u32>(), c->stream);
    b.mread_ok = true;
}
static void ensure_mread(mdbg_ctx* c) { for (Batch& b : c->batches) fill_mread_of(c, b); }

// Windows of every resident batch that has not been inserted yet -> counting table.  All pending batches go in one
// round: count their windows, check the capacity rule on the device, launch the inserts back to back, ONE host round
// trip at the end (the insert kernels do nothing if the table has to grow first; then it is grown and the round repeats).
// allow_pending: reserved regions may be waiting for their data (the multi-GPU layer inserts what has landed while the next round
// travels): only committed batches are touched, the regions in flight are not registered yet.
int insert_resident_impl(mdbg_ctx* c, bool allow_pending) {
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed) return fail(c, MDBG_E_STATE, "table holds routed records; local insertion is not allowed");
    if (c->pending_m && !allow_pending) return fail(c, MDBG_E_STATE, "reserved sketch regions have not been committed");
    hipStream_t s = c->stream;
    const size_t first = c->batches_inserted, last = c->batches.size();
    c->nodes_ok = false; c->ulist_ok = false;      // the table is about to change: edges need a new finalize
    bool any = false;
    for (size_t i = first; i < last; ++i) any = any || c->batches[i].m1 > c->batches[i].m0;
    c->batches_inserted = last;
    if (!any) return MDBG_OK;
    u64 sc[SC_N];
    // exact number of occurrences the round will insert (sizes the table): counted here, unless every batch came with the
    // number of its windows this rank owns (counted once by the rank that sketched it: mdbg_owner_counts / mdbg_sketch_commit)
    bool counts_known = c->own_world > 1;
    u64 known = 0;
    for (size_t i = first; i < last; ++i) { const Batch& b = c->batches[i]; if (b.m1 == b.m0) continue; if (b.owned == ~0ull) counts_known = false; else known += b.owned; }
    for (size_t i = first; i < last; ++i) {      // batches that will be scanned (no list, or their windows have to be counted first) need their whole map
        Batch& b = c->batches[i];
        if (!counts_known || !(b.list_off != ~0ull && b.owned != ~0ull && c->own_world > 1)) fill_mread_of(c, b);
    }
    if (counts_known) {
        c->h_known = known;
        HIPCHK(c, hipMemcpyAsync(scal(c) + SC_BATCHWIN, &c->h_known, 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->shards.as<u64>() + SH_OWNINS * CTR_SHARDS, 0, CTR_SHARDS * 8, s));
    } else {
        if (!c->batchwin_zero) HIPCHK(c, hipMemsetAsync(scal(c) + SC_BATCHWIN, 0, 8, s));
        if (c->own_world > 1) HIPCHK(c, hipMemsetAsync(c->shards.as<u64>() + SH_OWNED * CTR_SHARDS, 0, 2 * CTR_SHARDS * 8, s));      // SH_OWNED, SH_OWNINS
        for (size_t i = first; i < last; ++i) {
            const Batch& b = c->batches[i];
            if (b.m1 == b.m0) continue;
            if (c->own_world > 1)              // only the windows this context owns
                launch_count_owned_windows(c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, c->own_world, owner_thr(c, c->own_world), c->own_rank,
                                           c->shards.as<u64>() + SH_OWNED * CTR_SHARDS, s);
            else launch_count_windows(c->roff.as<u64>(), b.slot0, b.n_reads, c->P.k, scal(c) + SC_BATCHWIN, s);
        }
        if (c->own_world > 1) launch_sum_shards(c->shards.as<u64>() + SH_OWNED * CTR_SHARDS, 1, scal(c) + SC_BATCHWIN, s);
    }
    c->batchwin_zero = false;              // it holds this round's count from here on
    int e;
    u32* const flags = (u32*)(scal(c) + SC_CAPERR);                // [0] window index overflow, [1] table too small
    // Dense settings: far more windows than keys.  A table for "every window a new key" would be tens of GB (2 Gbases at the reference CLI's defaults:
    // 283 M windows, 19.6 M keys, 13.6 GB), so such rounds go in slices of window starts, each checked on the device against the keys the table holds
    // by then; the table grows (doubling) when a slice does not fit and the round resumes at that slice.
    u64 total_idx = 0;
    for (size_t i = first; i < last; ++i) total_idx += c->batches[i].m1 - c->batches[i].m0;
    u64 slice = 32ull << 20;
    { const char* sv = getenv("MDBG_INSERT_SLICE"); if (sv) { const u64 v = strtoull(sv, nullptr, 10); if (v) slice = std::max<u64>(v, (u64)OWN_SPAN); } }
    slice = (slice + OWN_SPAN - 1) / OWN_SPAN * OWN_SPAN;
    if (c->own_world <= 1 && total_idx > 2 * slice) {
        struct Sl { size_t b; u64 a, hi; };
        std::vector<Sl> sl;
        for (size_t i = first; i < last; ++i) { const Batch& b = c->batches[i]; for (u64 a = b.m0; a < b.m1; a += slice) sl.push_back({i, a, std::min(a + slice, b.m1)}); }
        if (c->cap < slots_for(c->n_distinct + slice)) { e = table_reserve(c, slice); if (e) return e; }
        size_t next = 0;
        for (;;) {
            { ZeroList z{}; z.p[0] = scal(c) + SC_CAPERR; z.n[0] = 0; z.set_p = scal(c) + SC_SLICEFAIL; z.set_v = ~0ull; launch_zero_regions(z, s); }
            HIPCHK(c, hipMemsetAsync(flags + 1, 0, 4, s));
            STAGE_EVENT(c, c->ev0, s);
            for (size_t j = next; j < sl.size(); ++j) {
                const Batch& b = c->batches[sl[j].b];
                launch_slice_check(c->shards.as<u64>(), scal(c) + SC_NDISTINCT, sl[j].hi - sl[j].a, c->cap, flags + 1, scal(c) + SC_SLICEFAIL, (u64)j, s);
                launch_insert_windows(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), sl[j].a, b.m1, b.slot0, b.first_ordinal,
                                      scal(c) + SC_NWINDOWS, flags, s, nullptr, sl[j].hi - sl[j].a);
            }
            STAGE_EVENT(c, c->ev1, s);
            e = read_scalars(c, sc); if (e) return e;
            c->ms_insert += ev_ms(c);
            c->n_distinct = sc[SC_NDISTINCT];
            if (!(sc[SC_CAPERR] >> 32)) break;
            if (sc[SC_SLICEFAIL] >= sl.size() || sc[SC_SLICEFAIL] < next) return fail(c, MDBG_E_DEVICE, "slice bookkeeping of the insertion is inconsistent");
            next = (size_t)sc[SC_SLICEFAIL];
            e = table_reserve(c, slice); if (e) return e;                 // at least doubles
        }
        if ((u32)sc[SC_PROBEERR]) return fail(c, MDBG_E_PARAM, "the table filled up during insertion");
        c->n_windows += sc[SC_BATCHWIN];
        if (sc[SC_IMPORTERR]) return fail(c, MDBG_E_PARAM, "read offsets of an imported sketch are not consistent with its size");
        if ((u32)sc[SC_CAPERR]) return fail(c, MDBG_E_CAPACITY, "a read has more than 2^26 minimizers");
        return MDBG_OK;
    }
    if (c->cap == 0) {                     // no table yet: size it from the data
        e = read_scalars(c, sc); if (e) return e;
        c->n_distinct = sc[SC_NDISTINCT];
        if (sc[SC_IMPORTERR]) return fail(c, MDBG_E_PARAM, "read offsets of an imported sketch are not consistent with its size");
        if (!sc[SC_BATCHWIN]) {
            // not a single window (every read has at most k minimizers): no table, no insertion kernel — and so nobody writes these batches' bytes of the claim map,
            // which a later finalize reads for EVERY index of the store (found by the multi-rank fuzz on recycled memory: a fresh hipMalloc hides it)
            if (c->claim.p) for (size_t i = first; i < last; ++i) { const Batch& b = c->batches[i]; if (b.m1 > b.m0) HIPCHK(c, hipMemsetAsync(c->claim.as<u8>() + b.m0, 0, b.m1 - b.m0, s)); }
            return MDBG_OK;
        }
        e = table_reserve(c, sc[SC_BATCHWIN]); if (e) return e;
    }
    for (;;) {
        launch_reserve_check(c->shards.as<u64>(), scal(c) + SC_NDISTINCT, scal(c) + SC_BATCHWIN, c->cap, flags + 1, s);
        STAGE_EVENT(c, c->ev0, s);
        // a listed batch's pairs and their segments in own_lists; per_entry: launch_insert_listed takes the per-entry kernel for it (the one decision behind the
        // grouping, the claim bytes and the launch below)
        auto list_of = [&](const Batch& b) { return c->own_lists.as<u32>() + b.list_off; };
        auto seg_of = [&](const Batch& b) { return c->own_lists.as<u32>() + b.list_off + 2 * b.owned; };
        auto per_entry = [&](const Batch& b) { return listed_per_entry(table_args(c), b.m0, b.m1, b.owned, seg_of(b) != nullptr); };
        // thinly listed batches (a rank's share of the peers' sketches at 4+ ranks) share ONE launch
        std::vector<ListedBatch> multi; u64 multi_total = 0;
        for (size_t i = first; i < last; ++i) {
            const Batch& b = c->batches[i];
            if (b.list_off != ~0ull && b.owned != ~0ull && b.owned && c->own_world > 1 && per_entry(b)) {
                ListedBatch lb{}; lb.start = multi_total; lb.m0 = b.m0; lb.m1 = b.m1; lb.first_ordinal = b.first_ordinal; lb.list = list_of(b);
                lb.slot0 = b.slot0; lb.n_reads = b.n_reads;
                multi.push_back(lb); multi_total += b.owned;
            }
        }
        if (multi.size() < 2) { multi.clear(); multi_total = 0; }
        // the per-entry kernel sets the claim byte of a window that creates its key and nothing else: the bytes of such a batch start from zero (the span kernels write
        // every byte of their batch themselves)
        if (c->claims_ok && c->claim.p && c->own_world > 1)
            for (size_t i = first; i < last; ++i) {
                const Batch& b = c->batches[i];
                if (b.list_off != ~0ull && b.owned != ~0ull && b.m1 > b.m0 && (!b.owned || per_entry(b)))
                    HIPCHK(c, hipMemsetAsync(c->claim.as<u8>() + b.m0, 0, b.m1 - b.m0, s));
            }
        if (!multi.empty()) {
            ListedBatch end{}; end.start = multi_total; multi.push_back(end);
            HIPCHK(c, c->listed_multi.ensure(multi.size() * sizeof(ListedBatch), 0, s));
            c->listed_multi_host = multi;                  // (stays alive until the copy has run: the round's closing read_scalars waits for the stream)
            HIPCHK(c, hipMemcpyAsync(c->listed_multi.p, c->listed_multi_host.data(), multi.size() * sizeof(ListedBatch), hipMemcpyHostToDevice, s));
            launch_insert_listed_multi(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), c->listed_multi.as<ListedBatch>(), (u32)multi.size() - 1, multi_total, flags, s);
        }
        for (size_t i = first; i < last; ++i) {
            const Batch& b = c->batches[i];
            if (multi_total && b.list_off != ~0ull && b.owned != ~0ull && b.owned && c->own_world > 1 && per_entry(b)) continue;      // went with the shared launch
            if (b.list_off != ~0ull && b.owned != ~0ull && c->own_world > 1)          // the sender listed this rank's windows: no scan of the foreign sketch
                launch_insert_listed(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, list_of(b), seg_of(b), b.owned, b.slot0, b.n_reads, b.first_ordinal, flags, s);
            else
                launch_insert_windows(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, b.slot0, b.first_ordinal,
                                      scal(c) + SC_NWINDOWS, flags, s);
        }
        STAGE_EVENT(c, c->ev1, s);
        if (c->own_world > 1) launch_sum_shards(c->shards.as<u64>() + SH_OWNINS * CTR_SHARDS, 1, scal(c) + SC_OWNINS, s);
        e = read_scalars(c, sc); if (e) return e;
        if (!(sc[SC_CAPERR] >> 32)) break;
        e = table_reserve(c, sc[SC_BATCHWIN]); if (e) return e;          // n_distinct is unchanged: nothing was inserted
    }
    if ((u32)sc[SC_PROBEERR] || (counts_known && sc[SC_OWNINS] != known))
        return fail(c, MDBG_E_PARAM, "the owned-window counts passed with the imported sketches do not match their contents");
    c->ms_insert += ev_ms(c);
    c->n_windows += sc[SC_BATCHWIN];
    c->n_distinct = sc[SC_NDISTINCT];
    // offsets of imported regions are validated on the device (mdbg_sketch_commit; clamped, so the kernels above stayed in bounds)
    if (sc[SC_IMPORTERR]) return fail(c, MDBG_E_PARAM, "read offsets of an imported sketch are not consistent with its size");
    if ((u32)sc[SC_CAPERR]) return fail(c, MDBG_E_CAPACITY, "a read has more than 2^26 minimizers");
    return MDBG_OK;
}

}  // namespace

extern "C" {

uint32_t mdbg_abi_version(void) { return MDBG_ABI_VERSION; }
uint32_t mdbg_build_flags(void) { return 0; }
static size_t host_cache_trim_fwd();
uint64_t mdbg_release_cached_memory(void) { (void)host_cache_trim_fwd(); return (uint64_t)block_cache().trim(); }

const char* mdbg_strerror(int err) {
    switch (err) {
        case MDBG_OK: return "ok";
        case MDBG_E_PARAM: return "invalid parameter";
        case MDBG_E_ALPHABET: return "Non-ACGTN nucleotide encountered";
        case MDBG_E_CAPACITY: return "capacity limit exceeded";
        case MDBG_E_DEVICE: return "HIP device error";
        case MDBG_E_NOMEM: return "out of memory";
        case MDBG_E_STATE: return "invalid state for this call";
        case MDBG_E_IO: return "file could not be opened or written";
        default: return "unknown error";
    }
}
const char* mdbg_last_error(mdbg_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

mdbg_ctx* mdbg_create(const mdbg_params* p, int* err) {
    int e = check_params(p);
    if (e) { if (err) *err = e; return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { if (err) *err = MDBG_E_DEVICE; return nullptr; }
    mdbg_ctx* c = new mdbg_ctx();
    c->P = *p;
    auto bail = [&](int code) -> mdbg_ctx* { if (err) *err = code; mdbg_destroy(c); return nullptr; };
    if (p->device >= 0) { if (hipSetDevice(p->device) != hipSuccess) return bail(MDBG_E_DEVICE); c->dev = p->device; }
    else if (hipGetDevice(&c->dev) != hipSuccess) return bail(MDBG_E_DEVICE);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(MDBG_E_DEVICE);
    for (auto& g : c->stage) if (hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking) != hipSuccess) return bail(MDBG_E_DEVICE);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return bail(MDBG_E_DEVICE);
    c->bound = make_hash_bound(p->density);
    if (c->d_t4.ensure((2 << (2 * BS_GS)) * 8, 0, c->stream) != hipSuccess) return bail(MDBG_E_NOMEM);
    { u64 t4[2 << (2 * BS_GS)]; bs_make_table<BS_GS>(t4); if (hipMemcpy(c->d_t4.p, t4, sizeof t4, hipMemcpyHostToDevice) != hipSuccess) return bail(MDBG_E_DEVICE); }
    if (c->scalars.ensure(SC_N * 8, 0, c->stream) != hipSuccess) return bail(MDBG_E_NOMEM);
    if (c->shards.ensure(N_SHARD_ARRAYS * CTR_SHARDS * 8, 0, c->stream) != hipSuccess) return bail(MDBG_E_NOMEM);
    if (hipMemset(c->shards.p, 0, N_SHARD_ARRAYS * CTR_SHARDS * 8) != hipSuccess) return bail(MDBG_E_DEVICE);
    if (hipMemset(c->scalars.p, 0, SC_N * 8) != hipSuccess) return bail(MDBG_E_DEVICE);
    if (c->roff.ensure(1024, 0, c->stream) != hipSuccess) return bail(MDBG_E_NOMEM);
    if (hipMemset(c->roff.p, 0, 8) != hipSuccess) return bail(MDBG_E_DEVICE);
    if (err) *err = MDBG_OK;
    return c;
}

void mdbg_destroy(mdbg_ctx* c) {          // the caller guarantees that no other call is in flight
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev3) (void)hipEventDestroy(c->ev3);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto e : c->tile_ev) (void)hipEventDestroy(e);
    if (c->eb) edge_buffers_destroy(c->eb);
    if (c->ub) unitig_buffers_destroy(c->ub);
    if (c->cb) contig_buffers_destroy(c->cb);
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    for (auto& g : c->stage) if (g.st) (void)hipStreamDestroy(g.st);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mdbg_sync(mdbg_ctx* c) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MDBG_OK;
}

int mdbg_copy_to_host(mdbg_ctx* c, void* dst, const void* d_src, uint64_t nbytes) {
    if (!c || (nbytes && (!dst || !d_src))) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nbytes) HIPCHK(c, hipMemcpy(dst, d_src, nbytes, hipMemcpyDeviceToHost));
    return MDBG_OK;
}
int mdbg_copy_to_device(mdbg_ctx* c, void* d_dst, const void* src, uint64_t nbytes) {
    if (!c || (nbytes && (!d_dst || !src))) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (nbytes) HIPCHK(c, hipMemcpy(d_dst, src, nbytes, hipMemcpyHostToDevice));
    return MDBG_OK;
}

int mdbg_sketch_device(mdbg_ctx* c, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    return sketch_device_impl(c, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal);
}

int mdbg_insert_resident(mdbg_ctx* c) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    return insert_resident_impl(c);
}

int mdbg_ingest_batch_device(mdbg_ctx* c, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    bool inserted = false;
    int e = sketch_device_impl(c, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal, true, &inserted);
    if (e) return e;
    return inserted ? MDBG_OK : insert_resident_impl(c);
}

// ---- host batch buffers that get page-locked on first use (mdbg_host_alloc, include/mdbg_hip.h) ---------------------------------------------------------
// hipMemcpyAsync from pageable memory is a memcpy into the runtime's staging buffers by ONE host thread, then DMA: 17 - 20 GB/s for batches that 16 reader
// threads have just written (the microbenchmark that re-sends one hot 64-MB buffer reaches 56; profiles/r05_f_pinned.json), i.e. 90 of the 190 ms of a
// 7-Gbase file -> .gfa run.  From page-locked memory it is one DMA at 57 GB/s.  hipHostMalloc takes 0.24 ms per MB (it faults every page in on the calling
// thread); hipHostRegister of pages that are resident already 0.011 ms per MB.  So: mdbg_host_alloc hands out ordinary page-aligned memory and remembers the
// range; the first ingest call that is given a pointer into it — by then the reader's threads have written, i.e. faulted, the batch — registers the whole
// range.  Nothing else changes for the caller; memory from elsewhere takes the staged path as before.
// Giving such a buffer back costs as much as page-locking it did not: unregistering + unmapping 73 MB took 10 ms, a reader's two ASCII buffers 67 ms of a 290-ms run.
// So mdbg_host_free keeps the range — registered — for the next mdbg_host_alloc of about that size, like the device block cache does: up to MDBG_HOST_CACHE_MB
// megabytes (default 2048, 0 = keep nothing); mdbg_release_cached_memory hands them back as well.
namespace {
struct HostRange { size_t bytes; int state; bool in_use; };      // state 0: not registered yet, 1: registered, 2: registration failed (pageable for good)
std::mutex g_host_mu;
std::map<uintptr_t, HostRange> g_host_ranges;
size_t g_host_cached = 0;
size_t host_cache_limit() {
    static const size_t lim = [] { const char* e = getenv("MDBG_HOST_CACHE_MB"); const long v = e ? atol(e) : 2048; return (size_t)(v < 0 ? 0 : v) << 20; }();
    return lim;
}
typedef std::pair<const uintptr_t, HostRange> HostEntry;
HostEntry* host_range_of(const void* p) {      // the range that holds p, or null; g_host_mu held
    auto it = g_host_ranges.upper_bound((uintptr_t)p);
    if (it == g_host_ranges.begin()) return nullptr;
    --it;
    return (uintptr_t)p < it->first + it->second.bytes ? &*it : nullptr;
}
void host_pin_if_known(const void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> l(g_host_mu);
    HostEntry* it = host_range_of(p);
    if (!it || !it->second.in_use || it->second.state != 0) return;
    it->second.state = hipHostRegister((void*)it->first, it->second.bytes, hipHostRegisterPortable) == hipSuccess ? 1 : 2;
    if (it->second.state == 2) (void)hipGetLastError();
}
void host_drop(std::map<uintptr_t, HostRange>::iterator it) {              // g_host_mu held
    if (it->second.state == 1) (void)hipHostUnregister((void*)it->first);
    free((void*)it->first);
    g_host_ranges.erase(it);
}
size_t host_cache_trim() {
    std::lock_guard<std::mutex> l(g_host_mu);
    size_t n = 0;
    for (auto it = g_host_ranges.begin(); it != g_host_ranges.end();) { auto cur = it++; if (!cur->second.in_use) { n += cur->second.bytes; host_drop(cur); } }
    g_host_cached = 0;
    return n;
}
}  // namespace
static size_t host_cache_trim_fwd() { return host_cache_trim(); }
void* mdbg_host_alloc(size_t bytes) {
    const size_t n = (std::max<size_t>(bytes, 1) + 4095) & ~(size_t)4095;
    {
        std::lock_guard<std::mutex> l(g_host_mu);
        auto best = g_host_ranges.end();
        for (auto it = g_host_ranges.begin(); it != g_host_ranges.end(); ++it)
            if (!it->second.in_use && it->second.bytes >= n && it->second.bytes <= n + n / 2 + (1u << 20) && (best == g_host_ranges.end() || it->second.bytes < best->second.bytes)) best = it;
        if (best != g_host_ranges.end()) { best->second.in_use = true; g_host_cached -= best->second.bytes; return (void*)best->first; }
    }
    void* p = nullptr;
    if (posix_memalign(&p, 4096, n) != 0 || !p) return nullptr;
    std::lock_guard<std::mutex> l(g_host_mu);
    g_host_ranges[(uintptr_t)p] = HostRange{n, 0, true};
    return p;
}
void mdbg_host_free(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> l(g_host_mu);
    auto it = g_host_ranges.find((uintptr_t)p);
    if (it == g_host_ranges.end() || !it->second.in_use) return;           // not from mdbg_host_alloc (or given back already): not ours to free
    if (it->second.state == 1 && g_host_cached + it->second.bytes <= host_cache_limit()) { it->second.in_use = false; g_host_cached += it->second.bytes; return; }
    host_drop(it);
}
int mdbg_host_is_pinned(const void* p) {
    std::lock_guard<std::mutex> l(g_host_mu);
    const HostEntry* it = host_range_of(p);
    return it && it->second.in_use && it->second.state == 1 ? 1 : 0;
}

// Copies a host batch into a free staging slot (waits for one), WITHOUT the context lock: the copy of one caller overlaps
// the kernels of another.  The slot is released by the StageHold destructor.
struct StageHold {
    mdbg_ctx* c = nullptr; Stage* g = nullptr;
    ~StageHold() { if (g) { { std::lock_guard<std::mutex> l(c->stage_mu); g->busy = false; } c->stage_cv.notify_one(); } }
};
static int stage_host_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, u64* n_bases_out, StageHold& hold) {
    if (!offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if (offsets[0] != 0) return fail(c, MDBG_E_PARAM, "offsets[0] must be 0");
    for (u64 r = 0; r < n_reads; ++r) {
        if (offsets[r + 1] < offsets[r]) return fail(c, MDBG_E_PARAM, "offsets must be non-decreasing");
        if (offsets[r + 1] - offsets[r] >= 0xFFFFFFFFull) return fail(c, MDBG_E_CAPACITY, "a read is longer than 2^32-1 bases");
    }
    const u64 nb = offsets[n_reads];
    if (nb && !bases) return fail(c, MDBG_E_PARAM, "null bases");
    {
        std::unique_lock<std::mutex> l(c->stage_mu);
        c->stage_cv.wait(l, [&] { return !c->stage[0].busy || !c->stage[1].busy; });
        hold.c = c; hold.g = c->stage[0].busy ? &c->stage[1] : &c->stage[0];
        hold.g->busy = true;
    }
    Stage* g = hold.g;
    (void)hipSetDevice(c->dev);
    HIPCHK(c, g->bases.ensure(nb + 64, 0, g->st));
    HIPCHK(c, g->off.ensure((n_reads + 1) * 8, 0, g->st));
    host_pin_if_known(bases);
    if (nb) HIPCHK(c, hipMemcpyAsync(g->bases.p, bases, nb, hipMemcpyHostToDevice, g->st));
    HIPCHK(c, hipMemcpyAsync(g->off.p, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, g->st));
    HIPCHK(c, hipStreamSynchronize(g->st));
    *n_bases_out = nb;
    return MDBG_OK;
}

// Thread-safe: several host threads may ingest concurrently.  Batches are ordered by first_read_ordinal, not by call
// time (the ordinals carry the order of the reference's sequential loop), so the result does not depend on interleaving.
int mdbg_ingest_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (n_reads == 0) return MDBG_OK;
    u64 nb = 0;
    StageHold hold;
    int e = stage_host_batch(c, bases, offsets, n_reads, &nb, hold); if (e) return e;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, first_read_ordinal); if (e) return e;
    return insert_resident_impl(c);
}

// ---- 2-bit packed input (see include/mdbg_hip.h) -------------------------------------------------------------
static int check_packed(mdbg_ctx* c, const mdbg_packed_batch* b) {
    if (!b) return fail(c, MDBG_E_PARAM, "null batch");
    if (b->n_reads && !b->offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if (b->n_exc && (!b->exc_pos || !b->exc_val)) return fail(c, MDBG_E_PARAM, "null exception list");
    return MDBG_OK;
}
static int packed_device_impl(mdbg_ctx* c, const mdbg_packed_batch* b, u64 n_bases, u64 first_ordinal, bool insert) {
    int e = check_packed(c, b); if (e) return e;
    if (n_bases && !b->words) return fail(c, MDBG_E_PARAM, "null packed words");
    SketchInput in; in.fmt = FMT_PLANES; in.d_planes = (const uint2*)b->words; in.d_exc_pos = b->exc_pos; in.d_exc_val = b->exc_val; in.n_exc = b->n_exc;
    bool inserted = false;
    e = sketch_device_impl(c, in, b->offsets, b->n_reads, n_bases, first_ordinal, insert, &inserted); if (e) return e;
    return insert && !inserted ? insert_resident_impl(c) : MDBG_OK;
}
int mdbg_ingest_batch_packed_device(mdbg_ctx* c, const mdbg_packed_batch* b, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    return packed_device_impl(c, b, n_bases, first_read_ordinal, true);
}
int mdbg_sketch_packed_device(mdbg_ctx* c, const mdbg_packed_batch* b, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    return packed_device_impl(c, b, n_bases, first_read_ordinal, false);
}
// host buffers: staged like mdbg_ingest_batch (a quarter of the bytes cross PCIe), several callers may overlap
int mdbg_ingest_batch_packed(mdbg_ctx* c, const mdbg_packed_batch* b, uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    { int e = check_packed(c, b); if (e) return e; }
    if (b->n_reads == 0) return MDBG_OK;
    if (b->offsets[0] != 0) return fail(c, MDBG_E_PARAM, "offsets[0] must be 0");
    for (u64 r = 0; r < b->n_reads; ++r) {
        if (b->offsets[r + 1] < b->offsets[r]) return fail(c, MDBG_E_PARAM, "offsets must be non-decreasing");
        if (b->offsets[r + 1] - b->offsets[r] >= 0xFFFFFFFFull) return fail(c, MDBG_E_CAPACITY, "a read is longer than 2^32-1 bases");
    }
    const u64 nb = b->offsets[b->n_reads], nw = (nb + 31) / 32;
    if (nb && !b->words) return fail(c, MDBG_E_PARAM, "null packed words");
    for (u64 i = 0; i < b->n_exc; ++i) if (b->exc_pos[i] >= nb || (i && b->exc_pos[i] <= b->exc_pos[i - 1])) return fail(c, MDBG_E_PARAM, "exception positions must be ascending and inside the batch");
    StageHold hold;
    {
        std::unique_lock<std::mutex> l(c->stage_mu);
        c->stage_cv.wait(l, [&] { return !c->stage[0].busy || !c->stage[1].busy; });
        hold.c = c; hold.g = c->stage[0].busy ? &c->stage[1] : &c->stage[0];
        hold.g->busy = true;
    }
    Stage* g = hold.g;
    (void)hipSetDevice(c->dev);
    HIPCHK(c, g->bases.ensure(nw * 8 + 64, 0, g->st));
    HIPCHK(c, g->off.ensure((b->n_reads + 1) * 8, 0, g->st));
    host_pin_if_known(b->words);
    if (nw) HIPCHK(c, hipMemcpyAsync(g->bases.p, b->words, nw * 8, hipMemcpyHostToDevice, g->st));
    HIPCHK(c, hipMemcpyAsync(g->off.p, b->offsets, (b->n_reads + 1) * 8, hipMemcpyHostToDevice, g->st));
    if (b->n_exc) {
        HIPCHK(c, g->exc_pos.ensure(b->n_exc * 8, 0, g->st)); HIPCHK(c, g->exc_val.ensure(b->n_exc, 0, g->st));
        HIPCHK(c, hipMemcpyAsync(g->exc_pos.p, b->exc_pos, b->n_exc * 8, hipMemcpyHostToDevice, g->st));
        HIPCHK(c, hipMemcpyAsync(g->exc_val.p, b->exc_val, b->n_exc, hipMemcpyHostToDevice, g->st));
    }
    HIPCHK(c, hipStreamSynchronize(g->st));
    MDBG_LOCK(c);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    mdbg_packed_batch d = *b;
    d.words = g->bases.as<u64>(); d.offsets = g->off.as<u64>(); d.exc_pos = g->exc_pos.as<u64>(); d.exc_val = g->exc_val.as<u8>();
    return packed_device_impl(c, &d, nb, first_read_ordinal, true);
}

int mdbg_pack_device(mdbg_ctx* c, const uint8_t* d_bases, uint64_t n_bases, uint64_t* d_words, uint64_t* d_exc_pos, uint8_t* d_exc_val,
                     uint64_t exc_cap, uint64_t* n_exc) {
    if (!c || !n_exc || (n_bases && (!d_bases || !d_words)) || (exc_cap && (!d_exc_pos || !d_exc_val))) return MDBG_E_PARAM;
    if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_words & 7)) return fail(c, MDBG_E_PARAM, "device pointers must be 16-byte (bases) / 8-byte (words) aligned");
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(scal(c) + SC_OVERMAX, 0, 8, s));           // scratch use of a scalar between sketch calls
    launch_pack_planes(d_bases, n_bases, (uint2*)d_words, d_exc_pos, d_exc_val, exc_cap, (unsigned long long*)(scal(c) + SC_OVERMAX), s);
    u64 n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, scal(c) + SC_OVERMAX, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *n_exc = n;
    if (n > exc_cap) return fail(c, MDBG_E_CAPACITY, "more bytes outside ACGT than the exception list holds");
    if (n > 1) {                                 // rare: order the side-list by position (host round trip; the list is short by nature)
        std::vector<u64> pos(n); std::vector<u8> val(n); std::vector<u64> idx(n);
        HIPCHK(c, hipMemcpy(pos.data(), d_exc_pos, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(val.data(), d_exc_val, n, hipMemcpyDeviceToHost));
        for (u64 i = 0; i < n; ++i) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](u64 a, u64 b) { return pos[a] < pos[b]; });
        std::vector<u64> p2(n); std::vector<u8> v2(n);
        for (u64 i = 0; i < n; ++i) { p2[i] = pos[idx[i]]; v2[i] = val[idx[i]]; }
        HIPCHK(c, hipMemcpy(d_exc_pos, p2.data(), n * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_exc_val, v2.data(), n, hipMemcpyHostToDevice));
    }
    return MDBG_OK;
}

int mdbg_sketch_only(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, const uint64_t** hashes,
                     const uint64_t** positions, const uint64_t** per_read_offsets, uint64_t* n_minimizers) {
    if (!c) return MDBG_E_PARAM;
    u64 nb = 0;
    StageHold hold;
    if (n_reads) { int e = stage_host_batch(c, bases, offsets, n_reads, &nb, hold); if (e) return e; }
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    c->so_hash.clear(); c->so_pos.clear(); c->so_off.assign(n_reads + 1, 0);
    if (n_reads) {
        int e;
        // sketch into the resident store, copy out, roll back (on every path: a failed copy must not leave the temporary batch behind)
        const u64 M0 = c->M, end0 = c->slot_end_m; const u32 slots0 = c->n_slots; const size_t nb0 = c->batches.size();
        const u64 sr = c->n_reads, sb = c->n_bases, st = c->n_tiles, ss = c->n_slow_tiles;
        const double ms0 = c->ms_sketch, mt0 = c->ms_tile; const u64 tl0 = c->n_tile_launches, tb0 = c->n_tile_bases;
        auto rollback = [&] {
            c->M = M0; c->n_slots = slots0; c->slot_end_m = end0; c->batches.resize(nb0);
            c->n_reads = sr; c->n_bases = sb; c->n_tiles = st; c->n_slow_tiles = ss;
            c->ms_sketch = ms0; c->ms_tile = mt0; c->n_tile_launches = tl0; c->n_tile_bases = tb0;
        };
        e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, 0);
        if (e) { rollback(); if (e == MDBG_E_ALPHABET) c->poisoned = 0; return e; }     // a bad byte in a sketch-only batch does not poison the node table; a device error does
        const u64 m = c->M - M0;
        c->so_hash.resize(m); std::vector<u32> p32(m);
        bool ok = hipStreamSynchronize(c->stream) == hipSuccess;
        if (ok && m) ok = hipMemcpy(c->so_hash.data(), c->mh.as<u64>() + M0, m * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(p32.data(), c->mpos.as<u32>() + M0, m * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) ok = hipMemcpy(c->so_off.data(), c->roff.as<u64>() + c->batches.back().slot0, (n_reads + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess;
        rollback();
        if (!ok) return fail(c, MDBG_E_DEVICE, "sketch_only: copy to the host");
        c->so_pos.resize(m);
        for (u64 i = 0; i < m; ++i) c->so_pos[i] = p32[i];
        for (auto& o : c->so_off) o -= M0;
    }
    if (hashes) *hashes = c->so_hash.data();
    if (positions) *positions = c->so_pos.data();
    if (per_read_offsets) *per_read_offsets = c->so_off.data();
    if (n_minimizers) *n_minimizers = c->so_hash.size();
    return MDBG_OK;
}

// --read_stats (src/main.rs:939-1004): per read of the batch, the abundance of each of its k-min-mers in the filtered node table
int mdbg_query_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, const uint32_t** counts,
                     const uint64_t** per_read_offsets, uint64_t* n_windows) {
    if (!c) return MDBG_E_PARAM;
    u64 nb = 0;
    StageHold hold;
    if (n_reads) { int e = stage_host_batch(c, bases, offsets, n_reads, &nb, hold); if (e) return e; }
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed) return fail(c, MDBG_E_STATE, "not available for a routed table");
    if (c->own_world > 1) return fail(c, MDBG_E_STATE, "not available for a partitioned table: k-min-mers owned by other ranks would read as absent");
    c->q_counts.clear(); c->q_off.assign(n_reads + 1, 0);
    if (n_reads) {
        // sketch into the resident store behind everything that is there, look the windows up, roll the store back
        const u64 M0 = c->M, end0 = c->slot_end_m; const u32 slots0 = c->n_slots; const size_t nb0 = c->batches.size();
        const u64 sr = c->n_reads, sb = c->n_bases, st = c->n_tiles, ss = c->n_slow_tiles;
        const double ms0 = c->ms_sketch, mt0 = c->ms_tile; const u64 tl0 = c->n_tile_launches, tb0 = c->n_tile_bases;
        int e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, 0);
        auto rollback = [&] {
            c->M = M0; c->n_slots = slots0; c->slot_end_m = end0; c->batches.resize(nb0);
            c->n_reads = sr; c->n_bases = sb; c->n_tiles = st; c->n_slow_tiles = ss;
            c->ms_sketch = ms0; c->ms_tile = mt0; c->n_tile_launches = tl0; c->n_tile_bases = tb0;
        };
        if (e) { rollback(); if (e == MDBG_E_ALPHABET) c->poisoned = 0; return e; }          // a bad byte in a query does not poison the node table; a device error does
        const Batch b = c->batches.back();
        const u64 m = b.m1 - b.m0;
        hipStream_t s = c->stream;
        std::vector<u32> per_min(m);
        std::vector<u64> roffs(n_reads + 1);
        if (m) {
            if (c->q_dev.ensure(m * 4, 0, s) != hipSuccess) { rollback(); return fail(c, MDBG_E_NOMEM, "query buffer"); }
            launch_query_windows(table_args(c), c->P.min_abundance, c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->q_dev.as<u32>(), s);
            if (hipMemcpyAsync(per_min.data(), c->q_dev.p, m * 4, hipMemcpyDeviceToHost, s) != hipSuccess) { rollback(); return fail(c, MDBG_E_DEVICE, "copy"); }
        }
        if (hipMemcpyAsync(roffs.data(), c->roff.as<u64>() + b.slot0, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { rollback(); return fail(c, MDBG_E_DEVICE, "copy"); }
        rollback();
        const u64 k = c->P.k;
        for (u64 r = 0; r < n_reads; ++r) {
            const u64 rs = roffs[r] - M0, re = roffs[r + 1] - M0;
            if (re - rs > k) for (u64 i = rs; i + k <= re; ++i) c->q_counts.push_back(per_min[i]);
            c->q_off[r + 1] = c->q_counts.size();
        }
    }
    if (counts) *counts = c->q_counts.data();
    if (per_read_offsets) *per_read_offsets = c->q_off.data();
    if (n_windows) *n_windows = c->q_counts.size();
    return MDBG_OK;
}

int mdbg_reset(mdbg_ctx* c, uint32_t new_k) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned == MDBG_E_DEVICE) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (new_k != 0 && new_k != c->P.k) for (const Batch& b : c->batches) if (b.partial)
        return fail(c, MDBG_E_STATE, "a resident foreign sketch holds only the hashes of this k's windows (mdbg_dist segments): ingest again, or exchange whole sketches (mdbg_dist_set_exchange)");
    c->poisoned = 0;
    int e = clear_table(c); if (e) return e;
    c->ms_sketch = c->ms_insert = c->ms_finalize = 0; c->ms_tile = 0; c->n_tile_launches = 0; c->n_tile_bases = 0;
    if (c->link_ctr.p) (void)hipMemsetAsync(c->link_ctr.p, 0, 8, c->stream);
    if (new_k == 0) {
        c->M = 0; c->n_slots = 0; c->slot_end_m = 0; c->pending_m = 0; c->batches.clear(); c->own_lists_n = 0;
        c->n_reads = c->n_bases = c->n_tiles = c->n_slow_tiles = 0;
        return MDBG_OK;
    }
    if (new_k < 2 || new_k > 4096) return fail(c, MDBG_E_PARAM, "bad k");
    if (new_k != c->P.k) for (Batch& b : c->batches) { b.owned = ~0ull; b.list_off = ~0ull; }      // the senders' window counts and lists were for the old k
    c->P.k = new_k;
    return insert_resident_impl(c);
}

int mdbg_set_lmer_filter(mdbg_ctx* c, const uint64_t* codes, uint64_t n) {
    if (!c || (n && !codes)) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!c->batches.empty()) return fail(c, MDBG_E_STATE, "set the l-mer filter before the first batch (or after mdbg_reset(ctx, 0))");
    if (!codes) { c->lmer_on = false; return MDBG_OK; }
    if (c->P.scheme != MDBG_SCHEME_DENSITY) return fail(c, MDBG_E_PARAM, "the l-mer filter belongs to the density scheme (src/read.rs:200-205)");
    if (c->P.l > 32) return fail(c, MDBG_E_PARAM, "the l-mer filter needs l <= 32");
    if (n >= (1ull << 40)) return fail(c, MDBG_E_CAPACITY, "l-mer set too large");
    u64 cap = 1024; while (cap < 2 * n + 2) cap <<= 1;
    std::vector<u64> tab(cap, LMERSET_EMPTY);
    const u64 mask = cap - 1, code_mask = c->P.l == 32 ? ~0ull : ((1ull << (2 * c->P.l)) - 1);
    u32 all_ones = 0;
    for (u64 i = 0; i < n; ++i) {
        const u64 code = codes[i];
        if (code & ~code_mask) return fail(c, MDBG_E_PARAM, "an l-mer code has bits above 2*l");
        if (code == LMERSET_EMPTY) { all_ones = 1; continue; }
        for (u64 h = lmerset_home(code, mask);; h = (h + 1) & mask) { if (tab[h] == code) break; if (tab[h] == LMERSET_EMPTY) { tab[h] = code; break; } }
    }
    HIPCHK(c, c->lmer_set.ensure(cap * 8, 0, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->lmer_set.p, tab.data(), cap * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // tab is about to go out of scope
    c->lmer_mask = mask; c->lmer_all_ones = all_ones; c->lmer_on = true;
    return MDBG_OK;
}

int mdbg_mark(mdbg_ctx* c, uint64_t* mark) {
    if (!c || !mark) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    if (c->pending_m) return fail(c, MDBG_E_STATE, "reserved sketch regions have not been committed");
    *mark = c->batches.size();
    return MDBG_OK;
}

int mdbg_rewind(mdbg_ctx* c, uint64_t mark) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned == MDBG_E_DEVICE) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->pending_m) return fail(c, MDBG_E_STATE, "reserved sketch regions have not been committed");
    if (mark > c->batches.size()) return fail(c, MDBG_E_PARAM, "not a mark of this context");
    c->poisoned = 0;
    int e = clear_table(c); if (e) return e;
    for (size_t i = mark; i < c->batches.size(); ++i) { c->n_reads -= std::min<u64>(c->n_reads, c->batches[i].n_reads); c->n_bases -= std::min<u64>(c->n_bases, c->batches[i].n_bases); }
    c->batches.resize(mark);
    c->batches_inserted = 0;                       // the table is empty again: everything kept is pending
    if (mark) { const Batch& b = c->batches.back(); c->M = b.m1; c->n_slots = b.slot0 + b.n_reads; c->slot_end_m = b.m1; }
    else { c->M = 0; c->n_slots = 0; c->slot_end_m = 0; c->own_lists_n = 0; }
    return MDBG_OK;
}

int mdbg_set_timing(mdbg_ctx* c, uint32_t level) {
    if (!c || level > 2) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    c->timing = (int)level;
    return MDBG_OK;
}

int mdbg_get_stats(mdbg_ctx* c, mdbg_stats* o) {
    if (!c || !o) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    memset(o, 0, sizeof *o);
    o->n_reads = c->n_reads; o->n_bases = c->n_bases; o->n_minimizers = c->M; o->n_windows = c->n_windows; o->n_distinct = c->n_distinct;
    o->table_capacity = c->cap; o->n_slow_tiles = c->n_slow_tiles; o->n_tiles = c->n_tiles;
    o->ms_sketch = c->ms_sketch; o->ms_insert = c->ms_insert; o->ms_finalize = c->ms_finalize;
    o->ms_sketch_tile = c->ms_tile; o->n_sketch_tile_launches = c->n_tile_launches; o->n_sketch_tile_bases = c->n_tile_bases;
    o->tile_bases = TILE_STRIDE;
    if (c->link_ctr.p) {
        (void)hipSetDevice(c->dev);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(&o->n_link_matches, c->link_ctr.p, 8, hipMemcpyDeviceToHost));
    }
    return MDBG_OK;
}

// FinArgs shared by finalize and the resolve_* entry points: batch table (sorted by first ordinal -> dense order of
// the ordinals), zeroed bitmaps over the resident minimizers, prefix buffers
static int fin_setup(mdbg_ctx* c, FinArgs& F, u64& n_words_out, bool byte_maps = false) {
    hipStream_t s = c->stream;
    c->nodes_ok = false; c->ulist_ok = false;
    F.ath_override = nullptr;
    const u32 k = c->P.k;
        // batches sorted by first ordinal -> dense order of the ordinals
        std::vector<Batch> bs = c->batches;
        std::sort(bs.begin(), bs.end(), [](const Batch& a, const Batch& b) { return a.first_ordinal < b.first_ordinal; });
        const u32 nb = (u32)bs.size();
        // the ordinal -> batch mapping below (and decode_ordinal / rep_ordinal on the device) needs disjoint ordinal ranges
        for (u32 i = 0; i + 1 < nb; ++i)
            if (bs[i].n_reads && bs[i].first_ordinal + bs[i].n_reads > bs[i + 1].first_ordinal) {
                char buf[200]; snprintf(buf, sizeof buf, "read ordinals of two batches overlap: [%llu, +%u) and [%llu, +%u) (first_read_ordinal must be the position of the batch's first record in the whole input)",
                                        (unsigned long long)bs[i].first_ordinal, bs[i].n_reads, (unsigned long long)bs[i + 1].first_ordinal, bs[i + 1].n_reads);
                return fail(c, MDBG_E_PARAM, buf);
            }
        std::vector<u64> fo(nb), rb(nb); std::vector<u32> nr(nb), s0(nb);
        u64 acc = 0;
        for (u32 i = 0; i < nb; ++i) { fo[i] = bs[i].first_ordinal; nr[i] = bs[i].n_reads; s0[i] = bs[i].slot0; rb[i] = acc; acc += bs[i].m1 - bs[i].m0; }
        // second view of the same batches, sorted by slot0 (= call order): slot -> read ordinal (rep_ordinal)
        std::vector<Batch> bs2 = c->batches;
        std::sort(bs2.begin(), bs2.end(), [](const Batch& a, const Batch& b) { return a.slot0 < b.slot0; });
        std::vector<u64> f2(nb), m2(nb), r2(nb); std::vector<u32> s2(nb);
        for (u32 i = 0; i < nb; ++i) { f2[i] = bs2[i].first_ordinal; s2[i] = bs2[i].slot0; }
        // third view, sorted by position in the store (regions reserved for peers are registered later than batches sketched after the
        // reservation, so this is not the slot order): minimizer index -> dense ordered index (dense_of_index)
        {
            std::vector<u32> ord(nb);
            for (u32 i = 0; i < nb; ++i) ord[i] = i;
            std::sort(ord.begin(), ord.end(), [&](u32 a, u32 b) { return bs[a].m0 != bs[b].m0 ? bs[a].m0 < bs[b].m0 : bs[a].m1 < bs[b].m1; });
            for (u32 i = 0; i < nb; ++i) { m2[i] = bs[ord[i]].m0; r2[i] = rb[ord[i]]; }
        }
        const size_t bt_bytes = (size_t)nb * (6 * 8 + 3 * 4);                   // u64 arrays first (alignment), then the u32 arrays
        HIPCHK(c, c->bt_dev.ensure(bt_bytes + 64, 0, s));
        u8* btp = c->bt_dev.as<u8>();
        // one staged copy; the staging vector belongs to the context, so no host sync is needed for its lifetime
        c->bt_host.resize(bt_bytes);
        u8* hp = c->bt_host.data();
        memcpy(hp, fo.data(), nb * 8); memcpy(hp + nb * 8, rb.data(), nb * 8); memcpy(hp + nb * 16, f2.data(), nb * 8);
        memcpy(hp + nb * 24, m2.data(), nb * 8); memcpy(hp + nb * 32, r2.data(), nb * 8);
        { std::vector<u64> m0o(nb); for (u32 i = 0; i < nb; ++i) m0o[i] = bs[i].m0; memcpy(hp + nb * 40, m0o.data(), nb * 8); }
        memcpy(hp + nb * 48, nr.data(), nb * 4); memcpy(hp + nb * 52, s0.data(), nb * 4); memcpy(hp + nb * 56, s2.data(), nb * 4);
        // uploaded only when it changed (a host that resets and ingests the same batches again — every step of the benchmark — finds the table of the step before in place:
        // the copy kernel and the gaps around it were ~0.03 ms of a 2.8-ms step)
        if (c->bt_sent_at != (const void*)btp || c->bt_sent.size() != bt_bytes || memcmp(c->bt_sent.data(), hp, bt_bytes) != 0) {
            HIPCHK(c, hipMemcpyAsync(btp, hp, bt_bytes, hipMemcpyHostToDevice, s));
            c->bt_sent = c->bt_host; c->bt_sent_at = (const void*)btp;
        }
        const u64 n_words = (c->M + 63) / 64; n_words_out = n_words;
        c->fin_bits = acc;
        const u64 n_blocks = (n_words + 1023) / 1024;
        HIPCHK(c, c->bm_first.ensure(n_words * 8, 0, s)); HIPCHK(c, c->bm_solid.ensure(n_words * 8, 0, s));
        HIPCHK(c, c->pre_first.ensure(n_words * 4, 0, s)); HIPCHK(c, c->pre_solid.ensure(n_words * 4, 0, s));
        HIPCHK(c, c->popc_tmp.ensure(n_blocks * 8 + 64, 0, s));
        {   // both bitmaps, SC_FIN0..2 and the three finalize shard arrays: one launch
            ZeroList z{};
            F.claims = 0;
            if (byte_maps) {                 // fin_mark marks in byte maps; the bitmaps are then written whole by launch_bytes_to_bits
                // The map of first sightings can start from the insertion's claim map (one byte per window start: "this window created its key") when every window
                // went through insert_windows_kernel with the map on and the dense order of the ordinals is the order of the store (batches ingested in
                // ordinal order, no gaps): fin_mark then only moves the marks of keys seen again whose first sighting is not their claimer.
                // Round 6: the same under a partitioned table and for batches whose dense order is not the store's (F.claims = 2): every insertion kernel of resident
                // windows writes its claims (a rank inserts only windows it owns, so "this window created its key" is as well defined as on one rank), the map is indexed by
                // store index and launch_claims_to_bits gathers it into the dense bitmaps.
                const bool use_claims = c->claims_ok && !c->routed && c->claim.p && c->batches_inserted == c->batches.size() && getenv("MDBG_NO_CLAIMS") == nullptr;
                bool dense_is_store = c->own_world <= 1 && acc == c->M;
                for (u32 i = 0; i < nb && dense_is_store; ++i) dense_is_store = !bs[i].partial && rb[i] == bs[i].m0;
                if (use_claims) {
                    F.claims = dense_is_store ? 1 : 2;
                    F.by_first = c->claim.as<u8>(); F.by_solid = nullptr;          // one map: bit 0 first sighting, bit 1 solid (fin_mark_claims_kernel); nothing to zero
                    z.n[0] = 0; z.n[1] = 0;                                        // (the bytes behind the store's end are masked by launch_bytes_to_bits: n_bits = M)
                } else {
                    HIPCHK(c, c->by_maps.ensure(n_words * 128, 0, s));
                    z.p[0] = c->by_maps.as<u64>(); z.n[0] = n_words * 16; z.n[1] = 0;
                    F.by_first = c->by_maps.as<u8>(); F.by_solid = F.by_first + n_words * 64;
                }
            } else { z.p[0] = c->bm_first.as<u64>(); z.n[0] = n_words; z.p[1] = c->bm_solid.as<u64>(); z.n[1] = n_words; }
            // the finalize counters: left clean by the finalize before (read_scalars(with_fin)) unless something went wrong in between or another user of fin_setup ran
            if (c->fin_dirty) { z.p[2] = scal(c) + SC_FIN0; z.n[2] = 3; z.p[3] = c->shards.as<u64>() + SH_FIN_WRAPPED * CTR_SHARDS; z.n[3] = 2 * CTR_SHARDS; }
            if (z.n[0] || z.n[1] || z.n[2]) launch_zero_regions(z, s);
            c->fin_dirty = true;              // from here until the counters have been published and zeroed again
        }
        F.tab = c->tab.as<Slot>(); F.cap = c->cap; F.mx = c->mx.as<u64>(); F.A = c->P.min_abundance; F.casc = cascade_of(F.A); F.k = k; F.l = c->P.l;
        F.mh = c->mh.as<u64>(); F.mpos = c->mpos.as<u32>(); F.roff = c->roff.as<u64>();
        F.bt.first_ordinal = (const u64*)btp; F.bt.rank_base = (const u64*)(btp + nb * 8); F.bt.by_slot_first = (const u64*)(btp + nb * 16);
        F.bt.by_m0 = (const u64*)(btp + nb * 24); F.bt.by_m0_rank = (const u64*)(btp + nb * 32);
        F.bt.m0 = (const u64*)(btp + nb * 40);
        F.bt.n_reads = (const u32*)(btp + nb * 48); F.bt.slot0 = (const u32*)(btp + nb * 52); F.bt.by_slot0 = (const u32*)(btp + nb * 56); F.bt.n = nb;
        F.mread = c->mread.as<u32>(); F.arena = c->arena.as<u64>();
        HIPCHK(c, c->solid_list.ensure((c->n_distinct + 1024) * 16, 0, s));
        F.solid_list = c->solid_list.as<u64>(); F.solid_dense = F.solid_list + (c->n_distinct + 1024); F.solid_count = scal(c) + SC_FIN0; F.order = nullptr;
        F.bm_first = c->bm_first.as<u64>(); F.bm_solid = c->bm_solid.as<u64>(); F.pre_first = c->pre_first.as<u32>(); F.pre_solid = c->pre_solid.as<u32>();
        F.sh_wrapped = c->shards.as<u64>() + SH_FIN_WRAPPED * CTR_SHARDS; F.sh_distinct = c->shards.as<u64>() + SH_FIN_DISTINCT * CTR_SHARDS;
    return MDBG_OK;
}

// finalize, phase 1: mark first sightings / solid nodes of THIS context's keys in the bitmaps, list the solid slots
// Nodes seen >= 65536 + minabund times: the reference's u16 abundance wrapped, and its entry describes sighting
// j* = A + 65536 * floor((count - A) / 65536) instead of the A-th (table.hip, wrap_list_kernel).  n_bound: upper bound of
// the number of such nodes.  Sets F.ath_override (null when there is none).  Rare and off the fast path: a table scan, a
// re-scan of the resident windows (or routed records), one segmented sort.
static int resolve_wrapped(mdbg_ctx* c, FinArgs& F, u64 n_bound, bool routed) {
    F.ath_override = nullptr;
    if (!n_bound) return MDBG_OK;
    hipStream_t s = c->stream;
    HIPCHK(c, c->w_jstar.ensure(n_bound * 8, 0, s)); HIPCHK(c, c->w_count.ensure(n_bound * 4, 0, s)); HIPCHK(c, c->w_ctr.ensure(16, 0, s));
    HIPCHK(c, hipMemsetAsync(c->w_ctr.p, 0, 16, s));
    launch_wrap_list(c->tab.as<Slot>(), c->cap, c->P.min_abundance, c->P.min_abundance > MDBG_CASCADE_MAX, c->w_jstar.as<u64>(), c->w_count.as<u32>(), (unsigned long long*)c->w_ctr.p, s);
    u64 h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->w_ctr.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const u64 n_w = h[0], total = h[1];
    if (!n_w) return MDBG_OK;
    if (total >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 occurrences of k-min-mers whose abundance wrapped");
    std::vector<u32> cnt(n_w), start(n_w + 1);
    HIPCHK(c, hipMemcpy(cnt.data(), c->w_count.p, n_w * 4, hipMemcpyDeviceToHost));
    start[0] = 0;
    for (u64 i = 0; i < n_w; ++i) start[i + 1] = start[i] + cnt[i];
    HIPCHK(c, c->w_start.ensure((n_w + 1) * 4, 0, s)); HIPCHK(c, c->w_fill.ensure(n_w * 4, 0, s)); HIPCHK(c, c->w_ath.ensure(n_w * 8, 0, s));
    HIPCHK(c, c->w_occ.ensure(total * 8, 0, s)); HIPCHK(c, c->w_sorted.ensure(total * 8, 0, s));
    HIPCHK(c, hipMemcpy(c->w_start.p, start.data(), (n_w + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->w_fill.p, 0, n_w * 4, s));
    const TableArgs T = table_args(c);
    if (routed) launch_wrap_scan_records(T, c->n_records, c->w_start.as<u32>(), c->w_fill.as<u32>(), c->w_occ.as<u64>(), s);
    else for (Batch& b : c->batches) {
        if (b.partial)          // only the listed windows' hashes are here: walk the list
            launch_wrap_scan_listed(T, c->mh.as<u64>(), c->roff.as<u64>(), b.m0, b.m1, c->own_lists.as<u32>() + b.list_off, b.owned, b.slot0, b.n_reads, b.first_ordinal,
                                    c->w_start.as<u32>(), c->w_fill.as<u32>(), c->w_occ.as<u64>(), s);
        else {
            fill_mread_of(c, b);
            launch_wrap_scan_windows(T, c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, b.slot0, b.first_ordinal,
                                     c->w_start.as<u32>(), c->w_fill.as<u32>(), c->w_occ.as<u64>(), s);
        }
    }
    if (!c->eb) c->eb = edge_buffers_create();
    HIPCHK(c, sort_segments_u64(c->eb, c->w_occ.as<u64>(), c->w_sorted.as<u64>(), total, (u32)n_w, c->w_start.as<u32>(), s));
    launch_wrap_pick((u32)n_w, c->w_start.as<u32>(), c->w_jstar.as<u64>(), c->w_sorted.as<u64>(), c->w_ath.as<u64>(), s);
    F.ath_override = c->w_ath.as<u64>();
    return MDBG_OK;
}

// fused: the caller runs phase 2 right away on the same stream (local finalize): no host sync in between, one timing span
static int finalize_begin_impl(mdbg_ctx* c, bool fused) {
    hipStream_t s = c->stream;
    c->fin_open = false;
    int e0 = fin_setup(c, c->finF, c->fin_words, true); if (e0) return e0;
    STAGE_EVENT(c, c->ev0, s);
    launch_fin_mark(c->finF, s);
    // (fused: the prefix kernel follows at once and takes the per-block popcounts from this launch; else the bitmaps are merged over the ranks first and counted afterwards)
    if (c->finF.claims == 2) launch_claims_to_bits(c->finF, c->fin_words, c->fin_bits, c->finF.bm_first, c->finF.bm_solid, s);
    else launch_bytes_to_bits(c->finF.by_first, c->finF.by_solid, c->fin_words, c->M, c->finF.bm_first, c->finF.bm_solid, fused ? c->popc_tmp.as<u32>() : nullptr, s);
    if (!fused) {
        // (partitioned: the caller merges the bitmaps over the ranks next; this rank's own solid bits give its rows their order, finalize_end_impl)
        HIPCHK(c, c->bm_local.ensure(c->fin_words * 8 + 8, 0, s));
        HIPCHK(c, hipMemcpyAsync(c->bm_local.p, c->finF.bm_solid, c->fin_words * 8, hipMemcpyDeviceToDevice, s));
        STAGE_EVENT(c, c->ev1, s);
        HIPCHK(c, hipStreamSynchronize(s));
        c->ms_finalize += ev_ms(c);
    }
    c->fin_open = true;
    return MDBG_OK;
}
// the rows are on the device (c->finF.o_*): hand them over as device pointers, or copied into the context's host vectors
static int finalize_hand_over(mdbg_ctx* c, mdbg_nodes* out, bool to_host, u64 n) {
    FinArgs& F = c->finF;
    const u32 k = c->P.k;
    if (!to_host) {
        out->keys = F.o_keys; out->index = F.o_index; out->abundance = F.o_abund; out->seqlen = F.o_seqlen; out->shift = F.o_shift;
        out->shift_full = F.o_shift_full; out->src_read = F.o_src_read; out->src_start = F.o_src_start; out->src_end = F.o_src_end; out->reversed = F.o_rev;
        return MDBG_OK;
    }
    const char* const what = "host copy of the node table";
    int e;
    if ((e = copy_out(c, c->h_keys, F.o_keys, n * k, what, &out->keys)) || (e = copy_out(c, c->h_index, F.o_index, n, what, &out->index)) ||
        (e = copy_out(c, c->h_abund, F.o_abund, n, what, &out->abundance)) || (e = copy_out(c, c->h_seqlen, F.o_seqlen, n, what, &out->seqlen)) ||
        (e = copy_out(c, c->h_shift, F.o_shift, 2 * n, what, &out->shift)) || (e = copy_out(c, c->h_shift_full, F.o_shift_full, 2 * n, what, &out->shift_full)) ||
        (e = copy_out(c, c->h_src_read, F.o_src_read, n, what, &out->src_read)) || (e = copy_out(c, c->h_src_start, F.o_src_start, n, what, &out->src_start)) ||
        (e = copy_out(c, c->h_src_end, F.o_src_end, n, what, &out->src_end)) || (e = copy_out(c, c->h_rev, F.o_rev, n, what, &out->reversed))) return e;
    return MDBG_OK;
}
// finalize, phase 2: ranks from the (possibly all-reduced) bitmaps, then the node rows of this context's solid keys.
// partitioned: rows are written compactly in list order and their global row goes to *d_row.
static int finalize_end_impl(mdbg_ctx* c, mdbg_nodes* out, bool to_host, bool partitioned, const uint64_t** d_row, uint64_t* n_solid_global, bool fused = false) {
    hipStream_t s = c->stream;
    const u32 k = c->P.k;
    FinArgs& F = c->finF;
    const u64 n_words = c->fin_words;
    c->fin_open = false;
    if (!fused) STAGE_EVENT(c, c->ev0, s);
    launch_popc_prefix2(F.bm_first, F.bm_solid, n_words, c->popc_tmp.as<u32>(), c->pre_first.as<u32>(), c->pre_solid.as<u32>(), s, fused && F.claims != 2);
    if (partitioned) launch_bitmap_totals(F.bm_first, F.pre_first, F.bm_solid, F.pre_solid, n_words, scal(c) + SC_TOTFIRST, s);      // popcounts of the merged bitmaps
    u64 sc[SC_N];
    int e;
    F.n_solid_dev = nullptr;
    // The number of solid nodes sizes the outputs and the last two launches, and reading it costs a host round trip in the middle of the stage.
    // When an earlier finalize of this context gives an estimate, the rows are written for the estimate straight away (the kernels take the true
    // count from the device and do nothing if it is larger) and the count is read once, at the end; wrong estimate or wrapped abundances: the
    // plain path below runs after all.
    const bool speculate = !partitioned && !c->before_emit && c->P.min_abundance <= MDBG_CASCADE_MAX && c->fin_rows_guess > 0;
    if (speculate) {
        const size_t cap_rows = c->fin_rows_guess;
        size_t off = 0; auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_keys = carve(cap_rows * k * 8), o_sf = carve(cap_rows * 16), o_sr = carve(cap_rows * 8), o_ss = carve(cap_rows * 8), o_se = carve(cap_rows * 8),
                     o_idx = carve(cap_rows * 4), o_sl = carve(cap_rows * 4), o_ab = carve(cap_rows * 2), o_sh = carve(cap_rows * 4), o_rv = carve(cap_rows);
        HIPCHK(c, c->fin_out.ensure(off + 256, 0, s)); HIPCHK(c, c->fin_order.ensure(cap_rows * 8, 0, s));
        u8* fo_ = c->fin_out.as<u8>();
        F.o_keys = (u64*)(fo_ + o_keys); F.o_shift_full = (u64*)(fo_ + o_sf); F.o_src_read = (u64*)(fo_ + o_sr); F.o_src_start = (u64*)(fo_ + o_ss);
        F.o_src_end = (u64*)(fo_ + o_se); F.o_index = (u32*)(fo_ + o_idx); F.o_seqlen = (u32*)(fo_ + o_sl); F.o_abund = (u16*)(fo_ + o_ab);
        F.o_shift = (u16*)(fo_ + o_sh); F.o_rev = fo_ + o_rv; F.o_row = nullptr;
        F.ath_override = nullptr; F.n_solid_dev = F.solid_count; F.order = nullptr;
        launch_fin_order(F, cap_rows, c->fin_order.as<u64>(), s);
        F.order = c->fin_order.as<u64>();
        launch_fin_emit(F, cap_rows, s);
        STAGE_EVENT(c, c->ev1, s);
        e = read_scalars(c, sc, true); if (e) return e;
        F.n_solid_dev = nullptr;
        if (sc[SC_FIN0] <= cap_rows && !sc[SC_FIN1]) {
            const u64 n_solid = sc[SC_FIN0];
            c->ms_finalize += ev_ms(c);
            out->n_wrapped = 0; out->n_distinct = sc[SC_FIN2];
            c->fin_rows_guess = n_solid + n_solid / 4 + 1024;
            if (d_row) *d_row = nullptr;
            out->n = n_solid;
            c->nodes_n = n_solid; c->nodes_ok = true; c->edges_ok = false;
            return finalize_hand_over(c, out, to_host, n_solid);
        }
        STAGE_EVENT(c, c->ev0, s);        // (the span of the plain path starts here; what was written above is overwritten)
    } else { e = read_scalars(c, sc, true); if (e) return e; }          // + wrapped, distinct; SC_FIN0 = solid count (list)
    const u64 n_solid = sc[SC_FIN0];
    c->fin_rows_guess = n_solid + n_solid / 4 + 1024;
    out->n_wrapped = sc[SC_FIN1]; out->n_distinct = sc[SC_FIN2];
    if (c->P.min_abundance > MDBG_CASCADE_MAX) { if (n_solid) { e = resolve_wrapped(c, F, n_solid, false); if (e) return e; } }      // every solid node: its A-th sighting from the re-scan
    else if (sc[SC_FIN1]) { e = resolve_wrapped(c, F, sc[SC_FIN1], false); if (e) return e; }
    if (partitioned) {                 // global totals = popcounts of the merged bitmaps
        out->n_distinct = sc[SC_TOTFIRST];
        if (n_solid_global) *n_solid_global = sc[SC_TOTSOLID];
    }
    // device outputs, one allocation
    const size_t n = n_solid;
    size_t off = 0; auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_keys = carve(n * k * 8), o_sf = carve(n * 16), o_sr = carve(n * 8), o_ss = carve(n * 8), o_se = carve(n * 8), o_row = carve(n * 8),
                 o_idx = carve(n * 4), o_sl = carve(n * 4), o_ab = carve(n * 2), o_sh = carve(n * 4), o_rv = carve(n);
    HIPCHK(c, c->fin_out.ensure(off + 256, 0, s));
    u8* fo_ = c->fin_out.as<u8>();
    F.o_keys = (u64*)(fo_ + o_keys); F.o_shift_full = (u64*)(fo_ + o_sf); F.o_src_read = (u64*)(fo_ + o_sr); F.o_src_start = (u64*)(fo_ + o_ss);
    F.o_src_end = (u64*)(fo_ + o_se); F.o_index = (u32*)(fo_ + o_idx); F.o_seqlen = (u32*)(fo_ + o_sl); F.o_abund = (u16*)(fo_ + o_ab);
    F.o_shift = (u16*)(fo_ + o_sh); F.o_rev = fo_ + o_rv; F.o_row = partitioned ? (u64*)(fo_ + o_row) : nullptr;
    if (c->before_emit) { e = c->before_emit(c->before_emit_self, F, n_solid); if (e) return e; }
    F.order = nullptr;
    if (!partitioned && n) {           // rows in index order: list the slots by row first, so that every output array is written front to back
        HIPCHK(c, c->fin_order.ensure(n * 8, 0, s));
        launch_fin_order(F, n, c->fin_order.as<u64>(), s);
        F.order = c->fin_order.as<u64>();
    } else if (partitioned && n && c->bm_local.p) {
        // The partition's rows in the order of their first sightings too (= ascending global row): the rank of a node among THIS rank's solid bits, from the copy of the
        // solid bitmap taken before the merge.  In list order (= slot order) the k values of every node's window were 280-byte reads scattered over the whole store:
        // fin_emit took 6.3 ms for the human table's 17.7 M nodes at one rank, 2.5 in index order (profiles/r06_notes.md).
        HIPCHK(c, c->pre_local.ensure(n_words * 4 + 8, 0, s)); HIPCHK(c, c->pre_local2.ensure(n_words * 4 + 8, 0, s));
        launch_popc_prefix2(c->bm_local.as<u64>(), c->bm_local.as<u64>(), n_words, c->popc_tmp.as<u32>(), c->pre_local.as<u32>(), c->pre_local2.as<u32>(), s);
        FinArgs FL = F; FL.bm_solid = c->bm_local.as<u64>(); FL.pre_solid = c->pre_local.as<u32>(); FL.n_solid_dev = nullptr;
        HIPCHK(c, c->fin_order.ensure(n * 8, 0, s));
        launch_fin_order(FL, n, c->fin_order.as<u64>(), s);
        F.order = c->fin_order.as<u64>();
    }
    launch_fin_emit(F, n, s);
    STAGE_EVENT(c, c->ev1, s);
    HIPCHK(c, hipStreamSynchronize(s));
    c->ms_finalize += ev_ms(c);
    if (d_row) *d_row = F.o_row;
    out->n = n_solid;
    c->nodes_n = n_solid; c->nodes_ok = !partitioned; c->edges_ok = false;
    return finalize_hand_over(c, out, to_host, n);
}

static int finalize_impl(mdbg_ctx* c, mdbg_nodes* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed) return fail(c, MDBG_E_STATE, "a routed table is finalized by the distributed driver (mdbg_routed_export / mdbg_resolve_* / mdbg_routed_keys)");
    memset(out, 0, sizeof *out);
    out->k = c->P.k;
    if (!(c->cap && c->M)) {
        c->h_keys.clear(); c->h_shift_full.clear(); c->h_src_read.clear(); c->h_src_start.clear(); c->h_src_end.clear();
        c->h_index.clear(); c->h_seqlen.clear(); c->h_abund.clear(); c->h_shift.clear(); c->h_rev.clear();
        return MDBG_OK;
    }
    int e = finalize_begin_impl(c, true); if (e) return e;
    return finalize_end_impl(c, out, to_host, false, nullptr, nullptr, true);
}
int mdbg_finalize(mdbg_ctx* c, mdbg_nodes* out) { return finalize_impl(c, out, true); }
int mdbg_finalize_device(mdbg_ctx* c, mdbg_nodes* out) { return finalize_impl(c, out, false); }
int mdbg_finalize_gfa(mdbg_ctx* c, mdbg_nodes* out) {
    int e = finalize_impl(c, out, false); if (e) return e;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    const u64 n = out->n;
    const uint32_t* d_index = out->index; const uint32_t* d_seqlen = out->seqlen; const uint16_t* d_abund = out->abundance;
    out->keys = nullptr; out->shift = nullptr; out->shift_full = nullptr; out->src_read = nullptr; out->src_start = nullptr; out->src_end = nullptr; out->reversed = nullptr;
    out->index = nullptr; out->seqlen = nullptr; out->abundance = nullptr;
    if (!(c->h_index.resize(n) && c->h_seqlen.resize(n) && c->h_abund.resize(n))) return fail(c, MDBG_E_NOMEM, "host copy of the node table");
    if (n) {
        HIPCHK(c, hipMemcpy(c->h_index.data(), d_index, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_seqlen.data(), d_seqlen, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_abund.data(), d_abund, n * 2, hipMemcpyDeviceToHost));
    }
    out->index = c->h_index.data(); out->seqlen = c->h_seqlen.data(); out->abundance = c->h_abund.data();
    return MDBG_OK;
}

int mdbg_nodes_digest(mdbg_ctx* c, const mdbg_nodes* nodes, uint64_t* sum, uint64_t* xr) {
    if (!c || !nodes || !sum || !xr) return MDBG_E_PARAM;
    if (nodes->n && (!nodes->keys || !nodes->abundance || !nodes->k)) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    hipStream_t s = c->stream;
    u64 h[2] = {0, 0};
    if (nodes->n) {
        HIPCHK(c, c->q_dev.ensure(16, 0, s));                         // (scratch of the query calls: between calls it holds nothing)
        HIPCHK(c, hipMemsetAsync(c->q_dev.p, 0, 16, s));
        launch_nodes_digest(nodes->keys, nodes->abundance, nodes->n, nodes->k, c->q_dev.as<u64>(), s);
        HIPCHK(c, hipMemcpyAsync(h, c->q_dev.p, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    *sum = h[0]; *xr = h[1];
    return MDBG_OK;
}

// ---- graph entry points (edges, unitigs, simplification, contigs): implemented in graph_api.inc -----------
#include "graph_api.inc"

// ---- replicated-sketch multi-GPU mode (see include/mdbg_hip.h) ---------------------------------------
int mdbg_set_partition(mdbg_ctx* c, uint32_t world, uint32_t rank) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    if (world < 1 || world > 4096 || rank >= world) return fail(c, MDBG_E_PARAM, "bad partition");
    if (c->n_distinct || c->batches_inserted) return fail(c, MDBG_E_STATE, "set the partition before inserting");
    c->own_world = world; c->own_rank = rank;
    return MDBG_OK;
}

int mdbg_sketch_view(mdbg_ctx* c, mdbg_sketch_store* out) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_minimizers = c->M; out->n_reads = c->n_slots;
    out->d_hashes = c->mh.as<u64>(); out->d_positions = c->mpos.as<u32>(); out->d_read_offsets = c->roff.as<u64>();
    return MDBG_OK;
}

int mdbg_ingest_sketch(mdbg_ctx* c, const uint64_t* d_hashes, const uint32_t* d_positions, const uint64_t* d_read_offsets, uint64_t n_reads,
                       uint64_t first_read_ordinal) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!n_reads) return MDBG_OK;
    if (!d_read_offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if ((u64)c->n_slots + n_reads >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many reads");
    hipStream_t s = c->stream;
    u64 ends[2] = {0, 0};
    HIPCHK(c, hipMemcpy(&ends[0], d_read_offsets, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&ends[1], d_read_offsets + n_reads, 8, hipMemcpyDeviceToHost));
    if (ends[1] < ends[0]) return fail(c, MDBG_E_PARAM, "offsets must be non-decreasing");
    const u64 m = ends[1] - ends[0];
    if (m && (!d_hashes || !d_positions)) return fail(c, MDBG_E_PARAM, "null sketch arrays");
    if (c->M + m >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers resident on one device");
    u32 slot0 = 0;
    { int e = next_slot0(c, c->M, n_reads, &slot0); if (e) return e; }
    if (c->M + m > c->mcap) { int e = store_ensure(c, c->M + m + 65536); if (e) return e; }
    if (m) {
        HIPCHK(c, hipMemcpyAsync(c->mh.as<u64>() + c->M, d_hashes + ends[0], m * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->mpos.as<u32>() + c->M, d_positions + ends[0], m * 4, hipMemcpyDeviceToDevice, s));
    }
    launch_rebase_offsets(d_read_offsets, (u32)n_reads, c->M - ends[0], c->roff.as<u64>() + slot0, s);
    launch_fill_mread(c->roff.as<u64>(), slot0, (u32)n_reads, c->mread.as<u32>(), s);
    HIPCHK(c, hipStreamSynchronize(s));
    Batch b; b.first_ordinal = first_read_ordinal; b.n_reads = (u32)n_reads; b.slot0 = slot0; b.m0 = c->M; b.m1 = c->M + m;
    c->batches.push_back(b);
    c->M += m; c->n_slots = slot0 + (u32)n_reads; c->slot_end_m = c->M;
    return MDBG_OK;
}

// ---- zero-copy import of peers' sketches (see include/mdbg_hip.h) -------------------------------------
int mdbg_store_reserve(mdbg_ctx* c, uint64_t n_minimizers, uint64_t n_reads) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (n_minimizers >= 0xFFFFFFF0ull || n_reads >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers or reads resident on one device");
    int e = store_ensure(c, n_minimizers); if (e) return e;
    HIPCHK(c, c->roff.ensure((n_reads + 2) * 8, ((u64)c->n_slots + 1) * 8, c->stream));
    return MDBG_OK;
}

int mdbg_sketch_reserve(mdbg_ctx* c, uint64_t n_minimizers, uint64_t** d_hashes, uint32_t** d_positions, uint64_t* region) {
    if (!c || !d_hashes || !d_positions || !region) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->M + n_minimizers >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers resident on one device");
    int e = store_ensure(c, c->M + n_minimizers); if (e) return e;
    *region = c->M;
    *d_hashes = c->mh.as<u64>() + c->M; *d_positions = c->mpos.as<u32>() + c->M;
    c->M += n_minimizers; c->pending_m += n_minimizers;
    return MDBG_OK;
}

static int sketch_commit_impl(mdbg_ctx* c, uint64_t region, uint64_t n_minimizers, const uint64_t* d_read_offsets, uint64_t n_reads, uint64_t first_read_ordinal,
                              uint64_t owned_windows, bool with_read_map) {
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (n_minimizers > c->pending_m || region + n_minimizers > c->M) return fail(c, MDBG_E_PARAM, "not a reserved region");
    if (n_reads && !d_read_offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if (first_read_ordinal + n_reads >= (1ull << (64 - WIN_BITS))) return fail(c, MDBG_E_CAPACITY, "read ordinal too large");
    c->pending_m -= n_minimizers;
    if (!n_reads) return MDBG_OK;
    hipStream_t s = c->stream;
    u32 slot0 = 0;
    { int e = next_slot0(c, region, n_reads, &slot0); if (e) return e; }
    // stream-ordered, no host round trip: the offsets (relative to the region, [0] = 0, [n_reads] = n_minimizers) are
    // checked on the device; a violation surfaces as MDBG_E_PARAM at the next insertion
    launch_rebase_offsets_checked(d_read_offsets, (u32)n_reads, region, n_minimizers, c->roff.as<u64>() + slot0, scal(c) + SC_IMPORTERR, s);
    if (with_read_map) launch_fill_mread(c->roff.as<u64>(), slot0, (u32)n_reads, c->mread.as<u32>(), s);
    Batch b; b.first_ordinal = first_read_ordinal; b.n_reads = (u32)n_reads; b.slot0 = slot0; b.m0 = region; b.m1 = region + n_minimizers;
    b.owned = owned_windows; b.mread_ok = with_read_map;
    c->batches.push_back(b);
    c->n_slots = slot0 + (u32)n_reads; c->slot_end_m = b.m1;
    return MDBG_OK;
}
int mdbg_sketch_commit(mdbg_ctx* c, uint64_t region, uint64_t n_minimizers, const uint64_t* d_read_offsets, uint64_t n_reads, uint64_t first_read_ordinal,
                       uint64_t owned_windows) {
    if (!c) return MDBG_E_PARAM;
    return sketch_commit_impl(c, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, owned_windows, true);
}

int mdbg_owner_counts(mdbg_ctx* c, uint32_t world, uint64_t* counts) {
    if (!c || !counts) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (world < 1 || world > 4096) return fail(c, MDBG_E_PARAM, "bad world");
    if (c->batches.empty()) return fail(c, MDBG_E_STATE, "no batch has been sketched or imported");
    Batch& b = c->batches.back();
    hipStream_t s = c->stream;
    fill_mread_of(c, b);
    HIPCHK(c, c->own_hist.ensure((size_t)world * 8, 0, s));
    HIPCHK(c, hipMemsetAsync(c->own_hist.p, 0, (size_t)world * 8, s));
    launch_owner_hist(c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, world, owner_thr(c, world), c->own_hist.as<u64>(), s);
    HIPCHK(c, hipMemcpyAsync(counts, c->own_hist.p, (size_t)world * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->own_world == world && c->batches_inserted < c->batches.size()) b.owned = counts[c->own_rank];      // this rank's own share
    return MDBG_OK;
}

// appends the n entries (pairs of u32, device memory) of the window list of a batch of n_min minimizers to the context's list storage, followed
// by the list's span segments (launch_list_segments) -> offset of the copy
static int keep_window_list(mdbg_ctx* c, const u32* d_list, u64 n, u64 n_min, u64* off) {
    hipStream_t s = c->stream;
    const u32 spans = owner_list_spans(n_min);
    HIPCHK(c, c->own_lists.ensure((c->own_lists_n + 2 * n + spans + 1 + 64) * 4, c->own_lists_n * 4, s));
    u32* const dst = c->own_lists.as<u32>() + c->own_lists_n;
    if (n) HIPCHK(c, hipMemcpyAsync(dst, d_list, n * 8, hipMemcpyDeviceToDevice, s));
    launch_list_segments(dst, n, spans, dst + 2 * n, s);
    *off = c->own_lists_n; c->own_lists_n += 2 * n + spans + 1;
    return MDBG_OK;
}

// which: index of the batch in c->batches, ~0 = the one registered last
// skip_own: this rank's own bucket is NOT part of *d_lists — the other buckets follow each other in rank order without it — and is not written anywhere: the multi-GPU
// layer never ships it, and the insertion of the rank's own batch finds the rank's windows itself (insert_windows_kernel: owner codes of the hashes it stages anyway).
// Rounds 3 - 5 wrote that bucket (8 bytes per window: 368 MB per 19.5-Gbase batch at one rank), cut it into spans and inserted from the list.  false: every bucket in
// *d_lists, the own one copied and kept as the batch's window list (mdbg_owner_lists' contract)
static int owner_lists_impl(mdbg_ctx* c, uint32_t world, uint64_t* counts, const uint32_t** d_lists, size_t which, bool skip_own = false) {
    if (!c || !counts || !d_lists) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (world < 1 || world > OWNL_MAX_WORLD) return fail(c, MDBG_E_PARAM, "owner lists are built for at most 64 ranks");
    if (c->batches.empty() || (which != ~(size_t)0 && which >= c->batches.size())) return fail(c, MDBG_E_STATE, "no batch has been sketched or imported");
    Batch& b = which == ~(size_t)0 ? c->batches.back() : c->batches[which];
    hipStream_t s = c->stream;
    fill_mread_of(c, b);
    const u64 n_min = b.m1 - b.m0;
    const u32 nb = (u32)((n_min + OWNL_SPAN - 1) / OWNL_SPAN);
    for (u32 d = 0; d < world; ++d) counts[d] = 0;
    *d_lists = nullptr;
    if (!nb) { if (c->own_world == world && c->batches_inserted < c->batches.size()) { b.owned = 0; b.list_off = skip_own ? ~0ull : c->own_lists_n; } return MDBG_OK; }
    HIPCHK(c, c->ol_owner.ensure(n_min + 64, 0, s));
    HIPCHK(c, c->ol_cnt.ensure((size_t)nb * world * 4, 0, s)); HIPCHK(c, c->ol_off.ensure((size_t)nb * world * 8, 0, s)); HIPCHK(c, c->ol_tot.ensure(OWNL_MAX_WORLD * 8, 0, s));
    launch_owner_list_count(c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, world, owner_thr(c, world), c->ol_cnt.as<u32>(), c->ol_owner.as<u8>(), s);
    launch_route_scan(c->ol_cnt.as<u32>(), nb, world, c->ol_off.as<u64>(), c->ol_tot.as<u64>(), s);
    HIPCHK(c, hipMemcpyAsync(counts, c->ol_tot.p, (size_t)world * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const bool keep = c->own_world == world && c->batches_inserted < c->batches.size();      // this rank keeps its own share of its own batch
    const bool skip = skip_own && keep;
    OwnerBases bases{}; u64 total = 0, all = 0;
    for (u32 d = 0; d < world; ++d) { bases.b[d] = total; all += counts[d]; if (!(skip && d == c->own_rank)) total += counts[d]; }
    if (all >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 windows in one batch");
    HIPCHK(c, c->ol_list.ensure((total + 64) * 8, 0, s));
    if (total) launch_owner_list_write(c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, world, owner_thr(c, world), b.slot0, c->ol_off.as<u64>(), bases, c->ol_list.as<u32>(), c->ol_owner.as<u8>(), s,
                                       skip ? c->own_rank : 0xFFFFFFFFu, nullptr);
    *d_lists = c->ol_list.as<u32>();
    if (skip) { b.owned = counts[c->own_rank]; b.list_off = ~0ull; }          // no list: insert_resident_impl takes insert_windows_kernel for this batch
    else if (keep) {
        u64 off = 0;
        int e = keep_window_list(c, c->ol_list.as<u32>() + 2 * bases.b[c->own_rank], counts[c->own_rank], n_min, &off); if (e) return e;
        b.owned = counts[c->own_rank]; b.list_off = off;
    }
    if (!skip_own) HIPCHK(c, hipStreamSynchronize(s));          // the lists are about to be read from other streams (the caller's send); the multi-GPU layer waits for the
                                                                 // stream once, right in front of its exchange (round_begin), not here as well
    return MDBG_OK;
}

int mdbg_owner_lists(mdbg_ctx* c, uint32_t world, uint64_t* counts, const uint32_t** d_lists) { return owner_lists_impl(c, world, counts, d_lists, ~(size_t)0); }

int mdbg_sketch_commit_listed(mdbg_ctx* c, uint64_t region, uint64_t n_minimizers, const uint64_t* d_read_offsets, uint64_t n_reads, uint64_t first_read_ordinal,
                              const uint32_t* d_list, uint64_t n_list) {
    if (!c || (n_list && !d_list)) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    const size_t nb0 = c->batches.size();
    int e = sketch_commit_impl(c, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, n_list, false); if (e) return e;      // the list names every window's read
    if (c->batches.size() == nb0) return MDBG_OK;                 // no reads: nothing was registered
    u64 off = 0;
    e = keep_window_list(c, d_list, n_list, n_minimizers, &off); if (e) return e;
    c->batches.back().list_off = off;
    return MDBG_OK;
}

// sync: wait for the stream first (the arrays are about to be read from other streams); false when the caller syncs later anyway
static int batch_info_impl(mdbg_ctx* c, mdbg_batch_info* out, size_t which, bool sync = true) {
    if (!c || !out) return MDBG_E_PARAM;
    if (c->batches.empty() || (which != ~(size_t)0 && which >= c->batches.size())) return fail(c, MDBG_E_STATE, "no batch has been sketched or imported");
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));      // the arrays are about to be read from other streams (RCCL send)
    const Batch& b = which == ~(size_t)0 ? c->batches.back() : c->batches[which];
    out->store_offset = b.m0; out->n_minimizers = b.m1 - b.m0; out->first_slot = b.slot0; out->n_reads = b.n_reads; out->first_read_ordinal = b.first_ordinal;
    out->d_hashes = c->mh.as<u64>() + b.m0; out->d_positions = c->mpos.as<u32>() + b.m0; out->d_read_offsets = c->roff.as<u64>() + b.slot0;
    return MDBG_OK;
}
int mdbg_last_batch(mdbg_ctx* c, mdbg_batch_info* out) { return batch_info_impl(c, out, ~(size_t)0); }

// Measurement hook (scratch/measure_rank_w8.py; no counterpart in the reference): what the multi-GPU layer spends on the SEGMENTS of this context's last batch — the sender's
// side (counts per list entry, their prefix, the packed hashes: pack_segments of dist_api.inc) and the receiver's (the same counts from the list, the hashes scattered to
// their places: scatter_segments), here into a scratch region.  counts / d_lists: as mdbg_owner_lists returned them (every bucket, the own one = `skip` ships nothing).
// out[0] = pack ms, out[1] = scatter ms, out[2] = list entries, out[3] = hashes packed.
int mdbg_dbg_segments_ms(mdbg_ctx* c, uint32_t world, uint32_t skip, const uint64_t* counts, const uint32_t* d_lists, double* out) {
    if (!c || !counts || !d_lists || !out || world < 1 || world > OWNL_MAX_WORLD) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->batches.empty()) return fail(c, MDBG_E_STATE, "no batch");
    const Batch& b = c->batches.back();
    hipStream_t s = c->stream;
    SegBuckets B{}; B.n = world; B.skip = skip;
    u64 total = 0;
    for (u32 r = 0; r < world; ++r) { B.start[r] = total; B.base[r] = b.m0; B.lim[r] = b.m1 - b.m0; total += counts[r]; }
    B.start[world] = total;
    out[0] = out[1] = 0; out[2] = (double)total; out[3] = 0;
    if (!total) return MDBG_OK;
    DevBuf tmp, misc, pay, scratch;
    HIPCHK(c, tmp.ensure((total / 1024 + 2) * 8, 0, s)); HIPCHK(c, misc.ensure((size_t)(OWNL_MAX_WORLD + 4) * 8, 0, s));
    HIPCHK(c, pay.ensure((b.m1 - b.m0) * 8 + 8, 0, s)); HIPCHK(c, scratch.ensure((b.m1 - b.m0) * 8 + 8, 0, s));      // (sized generously: the layer sizes the payload exactly, after its prefix)
    hipEvent_t e0, e1; HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
    u64 picks[OWNL_MAX_WORLD + 1] = {0};
    float best[2] = {1e30f, 1e30f};
    for (int rep = 0; rep < 3; ++rep)
        for (int side = 0; side < 2; ++side) {
            if (side) for (u32 r = 0; r < world; ++r) B.base[r] = 0;      // the receiver writes into the scratch region
            else for (u32 r = 0; r < world; ++r) B.base[r] = b.m0;
            HIPCHK(c, hipMemsetAsync(misc.p, 0, 8, s));
            HIPCHK(c, hipEventRecord(e0, s));
            launch_seg_prefix(d_lists, total, c->P.k, B, tmp.as<u64>(), misc.as<u64>(), misc.as<u64>() + 1, s);
            HIPCHK(c, hipMemcpyAsync(picks, misc.as<u64>() + 1, (size_t)(world + 1) * 8, hipMemcpyDeviceToHost, s));
            if (!side) HIPCHK(c, hipStreamSynchronize(s));                 // (the sender sizes its payload buffer from the prefix)
            launch_seg_copy(d_lists, total, c->P.k, B, tmp.as<u64>(), side ? scratch.as<u64>() : c->mh.as<u64>(), pay.as<u64>(), b.m1 - b.m0, side != 0, s);
            HIPCHK(c, hipEventRecord(e1, s));
            HIPCHK(c, hipStreamSynchronize(s));
            float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
            if (ms < best[side]) best[side] = ms;
        }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    out[0] = best[0]; out[1] = best[1]; out[3] = (double)picks[world];
    return MDBG_OK;
}

int mdbg_finalize_begin(mdbg_ctx* c, uint64_t** d_bm_first, uint64_t** d_bm_solid, uint64_t* n_words) {
    if (!c || !d_bm_first || !d_bm_solid || !n_words) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed) return fail(c, MDBG_E_STATE, "not available for a routed table");
    if (!c->M) {                       // no minimizer anywhere (empty input, or every read shorter than l): an empty table, not an error
        c->fin_open = true; c->fin_words = 0; c->nodes_ok = false;
        *d_bm_first = nullptr; *d_bm_solid = nullptr; *n_words = 0;
        return MDBG_OK;
    }
    if (!c->cap) { int e0 = table_reserve(c, 0); if (e0) return e0; }
    int e = finalize_begin_impl(c, false); if (e) return e;
    *d_bm_first = c->bm_first.as<u64>(); *d_bm_solid = c->bm_solid.as<u64>(); *n_words = c->fin_words;
    return MDBG_OK;
}

int mdbg_finalize_end(mdbg_ctx* c, mdbg_nodes* out, const uint64_t** d_row, uint64_t* n_nodes_global) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!c->fin_open) return fail(c, MDBG_E_STATE, "mdbg_finalize_begin was not called");
    memset(out, 0, sizeof *out);
    out->k = c->P.k;
    if (!c->fin_words) {               // see mdbg_finalize_begin: nothing resident
        c->fin_open = false;
        if (d_row) *d_row = nullptr;
        if (n_nodes_global) *n_nodes_global = 0;
        return MDBG_OK;
    }
    return finalize_end_impl(c, out, false, true, d_row, n_nodes_global);
}

int mdbg_synth_reads_device(mdbg_ctx* c, const mdbg_synth_params* sp, uint64_t first_read, const uint8_t** d_bases, const uint64_t** d_offsets, uint64_t* n_bases) {
    if (!c || !sp) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (sp->n_reads == 0 || sp->n_reads > 0x7FFFFFFFull || sp->genome_len == 0 || sp->min_len == 0 || sp->min_len > sp->max_len) return fail(c, MDBG_E_PARAM, "bad synth parameters");
    SynthP P; P.seed = sp->seed; P.genome_len = sp->genome_len; P.first_read = first_read; P.mean_len = sp->mean_len; P.sd_len = sp->sd_len;
    P.min_len = sp->min_len; P.max_len = sp->max_len; P.thr24 = (u32)(((u64)sp->err_ppm << 24) / 1000000ull);
    hipStream_t s = c->stream;
    HIPCHK(c, c->syn_lens.ensure(sp->n_reads * 8, 0, s));
    HIPCHK(c, c->syn_off.ensure((sp->n_reads + 1) * 8, 0, s));
    launch_synth(P, sp->n_reads, c->syn_lens.as<u64>(), c->syn_off.as<u64>(), nullptr, 0, s);
    u64 nb = 0;
    HIPCHK(c, hipMemcpyAsync(&nb, c->syn_off.as<u64>() + sp->n_reads, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, c->syn_bases.ensure(nb + 64, 0, s));
    launch_synth(P, sp->n_reads, c->syn_lens.as<u64>(), c->syn_off.as<u64>(), c->syn_bases.as<u8>(), 1, s);
    HIPCHK(c, hipStreamSynchronize(s));
    if (d_bases) *d_bases = c->syn_bases.as<u8>();
    if (d_offsets) *d_offsets = c->syn_off.as<u64>();
    if (n_bases) *n_bases = nb;
    return MDBG_OK;
}

}  // extern "C"

// ---- multi-GPU routing entry points: implemented in route_api.inc -------------------------------------
#include "route_api.inc"
