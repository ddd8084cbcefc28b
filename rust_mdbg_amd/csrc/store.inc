// store.inc — the resident sketch store: growth, the bookkeeping of its batches, the kept reads and the minimizer -> read map.
namespace {
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
// Bookkeeping: every write of M, n_slots, slot_end_m, pending_m and batches is in the functions from here to store_truncate.  store_append registers a batch whose minimizers are in place at [b.m0, b.m1); M follows when it extends the store (a committed region lies below M already)
void store_append(mdbg_ctx* c, const Batch& b) { c->batches.push_back(b); c->n_slots = b.slot0 + b.n_reads; c->slot_end_m = b.m1; c->M = std::max(c->M, b.m1); }
// n minimizers at the end of the store that await their data (mdbg_sketch_reserve) -> where they start; store_commit_region: n of them have arrived
u64 store_reserve_region(mdbg_ctx* c, u64 n) { const u64 region = c->M; c->M += n; c->pending_m += n; return region; }
void store_commit_region(mdbg_ctx* c, u64 n) { c->pending_m -= n; }
// What a temporary batch (mdbg_sketch_only, mdbg_query_batch) changes in the store and the stats.  StoreRollback takes it before the sketch and puts it back on
// every way out of its scope: nothing the batch did stays, a failed copy included.
struct StoreSnapshot { u64 M, slot_end_m; u32 n_slots; size_t n_batches; u64 n_reads, n_bases, n_tiles, n_slow_tiles; double ms_sketch, ms_tile; u64 n_tile_launches, n_tile_bases; };
StoreSnapshot store_snapshot(const mdbg_ctx* c) { return {c->M, c->slot_end_m, c->n_slots, c->batches.size(), c->n_reads, c->n_bases, c->n_tiles, c->n_slow_tiles, c->ms_sketch, c->ms_tile, c->n_tile_launches, c->n_tile_bases}; }
void store_restore(mdbg_ctx* c, const StoreSnapshot& s) {
    c->M = s.M; c->n_slots = s.n_slots; c->slot_end_m = s.slot_end_m; c->batches.resize(s.n_batches);
    c->n_reads = s.n_reads; c->n_bases = s.n_bases; c->n_tiles = s.n_tiles; c->n_slow_tiles = s.n_slow_tiles;
    c->ms_sketch = s.ms_sketch; c->ms_tile = s.ms_tile; c->n_tile_launches = s.n_tile_launches; c->n_tile_bases = s.n_tile_bases;
}
struct StoreRollback { mdbg_ctx* const c; const StoreSnapshot s; explicit StoreRollback(mdbg_ctx* c_) : c(c_), s(store_snapshot(c_)) {} ~StoreRollback() { store_restore(c, s); } };
// Forgets every batch behind the first n_batches, with its kept reads and its share of the read and base counts (mdbg_rewind; mdbg_reset(ctx, 0) keeps none).  The callers
// have cleared the table and hold no pending region: whatever stays is to be inserted again, and an empty store has neither window lists nor regions.
void store_truncate(mdbg_ctx* c, size_t n_batches) {
    for (size_t i = n_batches; i < c->batches.size(); ++i) { c->n_reads -= std::min<u64>(c->n_reads, c->batches[i].n_reads); c->n_bases -= std::min<u64>(c->n_bases, c->batches[i].n_bases); }
    c->batches.resize(n_batches); c->batches_inserted = 0;
    if (n_batches) { const Batch& b = c->batches.back(); c->M = b.m1; c->n_slots = b.slot0 + b.n_reads; c->slot_end_m = b.m1; }
    else { c->M = 0; c->n_slots = 0; c->slot_end_m = 0; c->pending_m = 0; c->own_lists_n = 0; }
}

// a device-resident batch (ASCII or 2-bit planes) as the sketch stage takes it
struct SketchInput {
    u32 fmt = FMT_ASCII;
    const u8* d_bases = nullptr;             // FMT_ASCII
    const uint2* d_planes = nullptr;         // FMT_PLANES: ceil(n_bases / 32) pairs
    const u64* d_exc_pos = nullptr; const u8* d_exc_val = nullptr; u64 n_exc = 0;   // FMT_PLANES: bytes outside ACGT, sorted by position
};

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
            HIPCHK(c, sort_exceptions(c->res.contigs.buf.get(), c->kp_exc_pos.as<u64>(), c->kp_exc_val.as<u8>(), k->exc_pos(), k->exc_val(), n, s));
        }
    } else HIPCHK(c, hipStreamSynchronize(s));
    out = std::move(k);
    return MDBG_OK;
}

// The minimizer -> read map of a batch that was imported with a window list is only written where the table needs it (the
// representatives, insert_listed_*); every other consumer asks for the whole map first.
static void fill_mread_of(mdbg_ctx* c, Batch& b) {
    if (b.mread_ok) return;
    launch_fill_mread(c->roff.as<u64>(), b.slot0, b.n_reads, c->mread.as<u32>(), c->stream);
    b.mread_ok = true;
}
}  // namespace
