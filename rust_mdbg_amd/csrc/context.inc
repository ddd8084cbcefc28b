// context.inc — the context (mdbg_ctx) and what every stage uses of it: errors, the lock, scalars, the owner function, the table, stage events; create / destroy
namespace {
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
               u64 adm_word = ~0ull;                                                        // counting pre-filter: where in mdbg_ctx::pf_adm the batch's admission bits of the running round start (~0: inserted ungated)
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

struct mdbg_ctx {
    std::recursive_mutex mu;                 // every entry point holds it while it touches the context
    std::mutex err_mu;                       // c->err may be written by callers that only hold a staging slot
    Stage stage[2]; std::mutex stage_mu; std::condition_variable stage_cv;
    mdbg_params P{};
    int dev = 0; hipStream_t stream = nullptr; std::string err; int poisoned = 0;
    u64 scal_seq = 0; bool batchwin_zero = false;      // batchwin_zero: SC_BATCHWIN is known to be 0 on the device
    u64* h_scal = nullptr;                   // pinned, device-visible: the scalars as the last read_scalars() published them
    u64 bound = 0; DevBuf d_t4;              // hash_bound (src/read.rs:183); 4-base tables of the exact evaluation
    // resident sketch store (every read ingested since create / reset(0)).  ONLY the store_* functions of store.inc write M, n_slots, slot_end_m, pending_m and batches (batches_inserted: they, the insertions, clear_table)
    DevBuf mh, mpos, mread, roff; u64 M = 0; u64 mcap = 0; u32 n_slots = 0;
    u64 slot_end_m = 0;                      // end (index into mh) of the batch that owns the last slot
    u64 pending_m = 0;                       // minimizers of reserved regions not yet committed (mdbg_sketch_reserve)
    std::vector<Batch> batches; size_t batches_inserted = 0;
    u64 h_known = 0;                         // staging of the known window count (insert_resident_impl)
    // sketch temporaries
    DevBuf bread, tile_recs, slab, n_valid, n_scan, last_read, tile_base, scan_tmp, gran_sum, tile_flags, scalars, phase_dbg, shards;   // shards: N_SHARD_ARRAYS x CTR_SHARDS u64 (SH_*)
    u32 slab_cap_min = 0;                    // grown when a tile's records did not fit its slab
    // node table
    DevBuf tab, mx; u64 cap = 0;
    // the counting pre-filter (MDBG_FLAG_PREFILTER; prefilter_api.inc).  ONLY the functions of prefilter_api.inc write these
    DevBuf pf_cells, pf_adm;                 // the filter (2 bits per cell), allocated at the first count; the admission bits of the batches of one insertion round
    u64 pf_n_cells = 0;                      // cells in force (0: no filter on this context)
    size_t pf_counted = 0;                   // batches [0, pf_counted) have been counted into the filter
    bool pf_stale = false, pf_dirty = false; // stale: the filter holds counts that no longer stand (a new k, a rewind): zero it and count every batch again;
                                             // dirty: a batch was counted since the last insertion round
    u64 n_windows_admitted = 0;
    // routed records
    DevBuf arena, route_out, route_tmp, route_h, route_f; u64 n_records = 0; bool routed = false;
    // finalize
    DevBuf by_maps;                          // fin_mark's byte maps (2 x 64 bytes per bitmap word)
    DevBuf link_ctr;                         // MDBG_COUNT_LINKS (test hook): one u64, see TableArgs::link_ctr
    DevBuf claim;                            // one byte per resident minimizer index: the window starting there created its key (TableArgs::claim); as large as the store
    bool claims_ok = false;                  // every window in the table was inserted by insert_windows_kernel with the claim map on (set by clear_table / the first table)
    size_t claims_fin_batches = 0; u64 claims_fin_top = 0;      // the last claim-map finalize of this table: how many batches it saw (0: none yet) and the largest first ordinal
                                             // among them.  It left marks on the first sightings it knew; a batch that comes later with a SMALLER first ordinal can move a
                                             // first sighting once more, and nothing clears the mark left on the old one: fin_setup then gives the claim map up (claims_ok)
    DevBuf bm_first, bm_solid, pre_first, pre_solid, popc_tmp, bt_dev, fin_out, solid_list, fin_order;
    DevBuf bm_local, pre_local, pre_local2;       // partitioned finalize: THIS rank's solid bitmap as it was before the merge over the ranks, and its prefix (the order of the partition's rows)
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
    DevBuf own_hist;                         // mdbg_owner_counts
    DevBuf own_lists; u64 own_lists_n = 0;   // window lists of the batches this context owns windows of (u32 each), see Batch::list_off
    DevBuf listed_multi; std::vector<ListedBatch> listed_multi_host;      // descriptors of the batches that share one listed-insertion launch
    DevBuf own_thr; u32 thr_world = 0, thr_k = 0; double thr_bound = 0;      // owner_thr()
    DevBuf ol_cnt, ol_off, ol_tot, ol_list, ol_owner;  // mdbg_owner_lists scratch / result
    DevBuf lmer_set; u64 lmer_mask = 0; bool lmer_on = false; u32 lmer_all_ones = 0;      // --lmer-counts: mdbg_set_lmer_filter
    DevBuf w_jstar, w_count, w_ctr, w_start, w_fill, w_occ, w_sorted, w_ath;   // nodes whose u16 abundance wrapped (resolve_wrapped)
    Results res;                             // what is derived from the table and kept for the caller, and which of it is current (results.inc)
    DevBuf kp_exc_pos, kp_exc_val, kp_cnt;   // keeping an ASCII batch: where the pack kernel appends the (unordered) exceptions, and their count
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
int fail_hip(mdbg_ctx* c, const char* what, hipError_t e) { return fail(c, e == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, what, e); }
#define MDBG_LOCK(c) std::lock_guard<std::recursive_mutex> lock_((c)->mu)
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail_hip((c), #call, e_); } while (0)
// how an entry point opens: its pointers checked, the lock taken (for the rest of the function), the context's device current, a poisoned context refused
#define MDBG_ENTER(c, args_ok) if (!(c) || !(args_ok)) return MDBG_E_PARAM; MDBG_LOCK(c); (void)hipSetDevice((c)->dev); if ((c)->poisoned) return fail((c), MDBG_E_STATE, "context is in an error state")
// Hands a list's columns to the caller, one col() per column: the device pointer as it is, or (to_host) the context's host copy `h` of the n elements at `dev`, filled by a
// blocking copy.  `what` names the list in an error; the first error stays in `err` and the columns behind it are left alone.
struct HandOver {
    mdbg_ctx* c; const char* what; bool to_host; int err = MDBG_OK;
    template <class T> void col(const T* dev, size_t n, HostRaw<T>& h, const T** dst) {
        if (err) return;
        if (!to_host) { *dst = dev; return; }
        if (!h.resize(n)) { err = fail(c, MDBG_E_NOMEM, what); return; }
        if (n) { const hipError_t e = hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost); if (e != hipSuccess) { err = fail_hip(c, what, e); return; } }
        *dst = h.data();
    }
};
bool nothing_resident(const mdbg_ctx* c) { return c->cap == 0 || c->M == 0; }      // no table yet, or no minimizer in the store: an empty context

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
        c->claims_fin_batches = 0;
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
    c->res.invalidate(FROM_NODES);
    // the key counter's shards, SC_NDISTINCT + SC_NWINDOWS, SC_IMPORTERR, SC_PROBEERR: zeroed by the launch that clears the table (stream-ordered, no host sync) — or by
    // a launch of their own when there is no table yet
    ZeroList z{};
    z.p[0] = c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS; z.n[0] = CTR_SHARDS; z.p[1] = scal(c) + SC_NDISTINCT; z.n[1] = 2;
    z.p[2] = scal(c) + SC_IMPORTERR; z.n[2] = 1; z.p[3] = scal(c) + SC_PROBEERR; z.n[3] = 1;
    if (c->cap) launch_clear_table(c->tab.as<Slot>(), c->cap, c->mx.as<u64>(), cascade_of(c->P.min_abundance) > 2 ? c->cap * (cascade_of(c->P.min_abundance) - 2) : 0, c->stream, &z);
    else launch_zero_regions(z, c->stream);
    c->n_distinct = 0; c->n_windows = 0; c->n_windows_admitted = 0; c->batches_inserted = 0; c->n_records = 0; c->routed = false;      // (the pre-filter's counts stay: they describe the resident batches)
    c->claims_ok = c->claim.p != nullptr; c->claims_fin_batches = 0;      // (an empty table: no finalize has left a mark in the claim map that the insertions will not rewrite)
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
    if ((p->flags & MDBG_FLAG_PREFILTER) && (p->min_abundance < 2 || p->prefilter_cells > PF_MAX_CELLS)) return MDBG_E_PARAM;      // (a singleton's fate depends on its cell: never a node)
    return MDBG_OK;
}
}  // namespace

extern "C" {
uint32_t mdbg_abi_version(void) { return MDBG_ABI_VERSION; }
uint32_t mdbg_build_flags(void) { return 0; }

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
    if (p->flags & MDBG_FLAG_PREFILTER) c->pf_n_cells = p->prefilter_cells ? p->prefilter_cells : PF_DEFAULT_CELLS;
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
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    for (auto& g : c->stage) if (g.st) (void)hipStreamDestroy(g.st);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                              // (with it the stages' buffers, Results)
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
}  // extern "C"
