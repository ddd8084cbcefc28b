// blocks.inc — memory the library holds on to: the process-wide cache of device blocks, DevBuf / HostRaw, host buffers page-locked on first use (mdbg_host_*)
namespace {
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

// ---- MDBG_GUARD (test hook): a fence around every block -------------------------------------------------------------------------------------
// No test that compares a stage's outputs can see a kernel that writes a few elements outside the buffer the host sized for it: the write lands in the slack of
// Buf::ensure / DevBuf::ensure, or in the up-to-twice-the-request of a cached block.  With MDBG_GUARD set every block is an allocation of its own, G + bytes + G, the
// payload exactly as large as the request (whoever adds slack asks mdbg_guard_mode() and adds none), poisoned like MDBG_POISON's, between two bands of
// BAND bytes that nobody may touch.  G = one workgroup's widest row of stores (256 lanes x 16 B); it keeps the alignment of the handed pointer, and both bands belong to
// the allocation, so what the guard catches has damaged nothing.  The bands are compared on every mdbg_guard_check and when the block is given back.  Writes only:
// a read outside a block leaves no trace.
struct GuardState {
    static constexpr size_t G = 4096;
    static constexpr int BAND = 0x5C;
    struct Blk { size_t bytes; int dev; };
    std::mutex mu; std::map<uintptr_t, Blk> live;      // base of the allocation -> its payload (handed out: base + G)
    uint64_t violations = 0; std::string first;
    // compares the host copy of one band with its pattern (mu held, the block's device current and idle).  A damaged band is counted once: it is reported and filled again.
    void judge_band(const unsigned char* h, uintptr_t band, const Blk& b, bool front) {
        size_t n_bad = 0, lo = G, hi = 0;
        for (size_t i = 0; i < G; ++i) if (h[i] != (unsigned char)BAND) { ++n_bad; lo = std::min(lo, i); hi = i; }
        if (!n_bad) return;
        ++violations;
        if (first.empty()) {         // the damaged byte next to the payload names the overrun: the first one behind the end, the last one in front
            char t[160];
            if (front) snprintf(t, sizeof t, "block of %zu bytes: byte -%zu in front (%zu damaged)", b.bytes, G - hi, n_bad);
            else snprintf(t, sizeof t, "block of %zu bytes: byte +%zu behind the end (%zu damaged)", b.bytes, lo, n_bad);
            first = t;
        }
        if (hipMemset((void*)band, BAND, G) != hipSuccess) (void)hipGetLastError();
        (void)hipDeviceSynchronize();
    }
    // one block, when it is given back
    void check_block(uintptr_t base, const Blk& b) {
        int cur = 0; (void)hipGetDevice(&cur);
        if (b.dev != cur) (void)hipSetDevice(b.dev);
        (void)hipDeviceSynchronize();
        unsigned char h[2 * G];
        if (hipMemcpy(h, (const void*)base, G, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(h + G, (const void*)(base + G + b.bytes), G, hipMemcpyDeviceToHost) == hipSuccess) {
            judge_band(h, base, b, true); judge_band(h + G, base + G + b.bytes, b, false);
        } else (void)hipGetLastError();
        if (b.dev != cur) (void)hipSetDevice(cur);
    }
    // every live block (mdbg_guard_check runs after every library call of a guarded test): per device one wait, the bands queued into one page-locked buffer, one more wait
    unsigned char* stage = nullptr; size_t stage_cap = 0;
    void check_all(uint64_t* n_blocks, uint64_t* n_bytes) {
        const size_t need = live.size() * 2 * G;
        if (need > stage_cap) {
            if (stage) (void)hipHostFree(stage);
            stage = nullptr; stage_cap = 0;
            if (hipHostMalloc((void**)&stage, 2 * need, hipHostMallocDefault) == hipSuccess) stage_cap = 2 * need; else (void)hipGetLastError();
        }
        int cur = 0; (void)hipGetDevice(&cur);
        std::vector<int> devs;
        for (const auto& b : live) { *n_blocks += 1; *n_bytes += b.second.bytes; if (std::find(devs.begin(), devs.end(), b.second.dev) == devs.end()) devs.push_back(b.second.dev); }
        if (need > stage_cap) { for (const auto& b : live) check_block(b.first, b.second); return; }
        for (int dev : devs) {
            if (dev != cur) (void)hipSetDevice(dev);
            (void)hipDeviceSynchronize();
            bool ok = true; size_t i = 0;
            for (const auto& b : live) {
                if (b.second.dev != dev) continue;
                ok = ok && hipMemcpyAsync(stage + i, (const void*)b.first, G, hipMemcpyDeviceToHost, nullptr) == hipSuccess
                        && hipMemcpyAsync(stage + i + G, (const void*)(b.first + G + b.second.bytes), G, hipMemcpyDeviceToHost, nullptr) == hipSuccess;
                i += 2 * G;
            }
            ok = ok && hipStreamSynchronize(nullptr) == hipSuccess;
            i = 0;
            for (const auto& b : live) {
                if (b.second.dev != dev) continue;
                if (ok) { judge_band(stage + i, b.first, b.second, true); judge_band(stage + i + G, b.first + G + b.second.bytes, b.second, false); }
                i += 2 * G;
            }
            if (!ok) (void)hipGetLastError();
            if (dev != cur) (void)hipSetDevice(cur);
        }
    }
};
inline GuardState& guard_state() { static GuardState* const g = new GuardState(); return *g; }
hipError_t guard_alloc(void** p, size_t bytes, size_t* cap) {
    constexpr size_t G = GuardState::G;
    int dev = 0; (void)hipGetDevice(&dev);
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, G + bytes + G);
    if (e != hipSuccess) return e;
    e = hipMemset(base, GuardState::BAND, G);
    if (e == hipSuccess && bytes) e = hipMemset(base + G, 0xA5, bytes);
    if (e == hipSuccess) e = hipMemset(base + G + bytes, GuardState::BAND, G);
    if (e == hipSuccess) e = hipDeviceSynchronize();      // (the fills run on the null stream, which the contexts' streams do not wait for)
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    GuardState& g = guard_state();
    { std::lock_guard<std::mutex> l(g.mu); g.live[(uintptr_t)base] = GuardState::Blk{bytes, dev}; }
    *p = base + G; *cap = bytes;
    return hipSuccess;
}
void guard_free(void* p) {      // in this order: wait for the device (check_block), compare both bands, forget the block, hipFree
    GuardState& g = guard_state();
    const uintptr_t base = (uintptr_t)p - GuardState::G;
    {
        std::lock_guard<std::mutex> l(g.mu);
        auto it = g.live.find(base);
        if (it == g.live.end()) { ++g.violations; if (g.first.empty()) g.first = "a block was given back that the guard did not hand out"; return; }
        g.check_block(base, it->second);
        g.live.erase(it);
    }
    (void)hipFree((void*)base);
}
}  // namespace
// read once; the places that add slack to a request (Buf::ensure in graph_common.h, both attempts of DevBuf::ensure) ask it; keep_batch (store.inc) asks for exactly its sizes
// already.  Hidden: not an export of the library.
__attribute__((visibility("hidden"))) bool mdbg_guard_mode() { static const bool on = getenv("MDBG_GUARD") != nullptr; return on; }
hipError_t mdbg_block_alloc(void** p, size_t bytes, size_t* cap) {
    if (mdbg_guard_mode()) return guard_alloc(p, bytes, cap);
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
    if (mdbg_guard_mode()) { guard_free(p); return; }
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
        const bool exact = mdbg_guard_mode();       // MDBG_GUARD: no slack, so that the first byte behind what the stage asked for is a band's
        hipError_t e = mdbg_block_alloc(&np, exact ? bytes : bytes + bytes / 4 + 256, &ncap);
        if (e != hipSuccess) { (void)hipGetLastError(); e = mdbg_block_alloc(&np, exact ? bytes : bytes + 256, &ncap); if (e != hipSuccess) return e; }
        if (p && keep) { e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, s); if (e != hipSuccess) { mdbg_block_free(np, ncap); return e; } (void)hipStreamSynchronize(s); }
        if (p) mdbg_block_free(p, cap);      // (every user of the old block was ordered before the copy or is done: callers grow a buffer only between its uses)
        p = np; cap = ncap;
        return hipSuccess;
    }
    void release() { if (p) mdbg_block_free(p, cap); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};
}  // namespace
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
extern "C" {
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
uint64_t mdbg_release_cached_memory(void) { (void)host_cache_trim(); return (uint64_t)block_cache().trim(); }
// ---- test hooks of MDBG_GUARD (include/mdbg_hip.h) ----
uint64_t mdbg_guard_check(uint64_t* n_blocks, uint64_t* n_bytes) {
    uint64_t nb = 0, by = 0, v = 0;
    if (mdbg_guard_mode()) {
        GuardState& g = guard_state();
        std::lock_guard<std::mutex> l(g.mu);
        g.check_all(&nb, &by);
        v = g.violations;
    }
    if (n_blocks) *n_blocks = nb;
    if (n_bytes) *n_bytes = by;
    return v;
}
const char* mdbg_guard_report(void) {
    if (!mdbg_guard_mode()) return "";
    GuardState& g = guard_state();
    std::lock_guard<std::mutex> l(g.mu);
    static std::string out;          // (the text outlives the lock; the first report only ever changes from empty to set, the self-test aside)
    out = g.first;
    return out.c_str();
}
// A check that cannot fail is no check: one byte behind the end of a 1000-byte block and one byte in front of it, both inside the block's own allocation, have
// to be counted and named.  The two planted violations are taken out of the count again.  0 = the guard works; -1 = guard mode is off; > 0 = the step that failed.
int mdbg_guard_selftest(void) {
    if (!mdbg_guard_mode()) { fprintf(stderr, "mdbg_guard_selftest: MDBG_GUARD is not set\n"); return -1; }
    GuardState& g = guard_state();
    void* p = nullptr; size_t cap = 0;
    if (mdbg_block_alloc(&p, 1000, &cap) != hipSuccess) { (void)hipGetLastError(); return 1; }
    uint64_t v0 = 0; std::string kept;
    { v0 = mdbg_guard_check(nullptr, nullptr); std::lock_guard<std::mutex> l(g.mu); kept.swap(g.first); }
    int bad = cap == 1000 ? 0 : 2;
    uint64_t nb = 0, by = 0;
    if (!bad && (hipMemset(p, 0, 1001) != hipSuccess || mdbg_guard_check(&nb, &by) != v0 + 1 || nb < 1 || by < 1000)) bad = 3;
    if (!bad && strstr(mdbg_guard_report(), "block of 1000 bytes: byte +0 behind the end") == nullptr) bad = 4;
    { std::lock_guard<std::mutex> l(g.mu); g.first.clear(); }
    if (!bad && (hipMemset((char*)p - 1, 0, 1) != hipSuccess || mdbg_guard_check(nullptr, nullptr) != v0 + 2)) bad = 5;
    if (!bad && strstr(mdbg_guard_report(), "block of 1000 bytes: byte -1 in front") == nullptr) bad = 6;
    if (!bad && mdbg_guard_check(nullptr, nullptr) != v0 + 2) bad = 7;          // an intact block adds nothing
    // both bands as they were, whatever happened above, so that giving the block back counts nothing
    if (hipMemset((char*)p - GuardState::G, GuardState::BAND, GuardState::G) != hipSuccess || hipMemset((char*)p + 1000, GuardState::BAND, GuardState::G) != hipSuccess) { (void)hipGetLastError(); if (!bad) bad = 8; }
    (void)hipDeviceSynchronize();
    { std::lock_guard<std::mutex> l(g.mu); g.violations = v0; g.first.swap(kept); }
    mdbg_block_free(p, cap);
    if (!bad && mdbg_guard_check(nullptr, nullptr) != v0) bad = 9;
    (void)hipGetLastError();
    return bad;
}
}  // extern "C"
