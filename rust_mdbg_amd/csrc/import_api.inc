// import_api.inc — what the multi-GPU layer builds on: the partition, sketch views and imports (copying and zero-copy), owner counts and lists.  Inside api.inc's extern "C".
// ---- replicated-sketch multi-GPU mode (see include/mdbg_hip.h) ---------------------------------------
int mdbg_set_partition(mdbg_ctx* c, uint32_t world, uint32_t rank) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    if (world < 1 || world > 4096 || rank >= world) return fail(c, MDBG_E_PARAM, "bad partition");
    if (world > 1 && prefilter_on(c)) return fail(c, MDBG_E_STATE, PF_UNAVAILABLE);
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
    store_append(c, b);
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
    *region = store_reserve_region(c, n_minimizers);
    *d_hashes = c->mh.as<u64>() + *region; *d_positions = c->mpos.as<u32>() + *region;
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
    store_commit_region(c, n_minimizers);
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
    store_append(c, b);      // (below M: it stays)
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
