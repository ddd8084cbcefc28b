// prefilter_api.inc — the host side of the counting pre-filter (MDBG_FLAG_PREFILTER; definition in include/mdbg_hip.h, kernels in prefilter.hip): the filter's life,
// the counting of the batches, and the two steps an insertion round takes from it — prefilter_prepare in front of the round, prefilter_admit in the place of the
// round's window count.  The round itself is insert_resident_impl's (ingest_api.inc).
namespace {
bool prefilter_on(const mdbg_ctx* c) { return c->pf_n_cells != 0; }
constexpr const char* PF_UNAVAILABLE = "not available on a context with the counting pre-filter (MDBG_FLAG_PREFILTER): one GPU, local insertion only";
// the admission bits of a batch in the running round (null: the batch is inserted ungated)
const u64* adm_of(const mdbg_ctx* c, const Batch& b) { return b.adm_word == ~0ull ? nullptr : c->pf_adm.as<u64>() + b.adm_word; }

// mdbg_reset(new_k), mdbg_rewind: counts cannot be taken back, so the next count zeroes the filter and takes every resident batch again
void prefilter_invalidate(mdbg_ctx* c) { if (prefilter_on(c)) { c->pf_stale = true; c->pf_counted = 0; } }
// mdbg_reset(ctx, 0)
void prefilter_drop(mdbg_ctx* c) { c->pf_cells.release(); c->pf_adm.release(); c->pf_counted = 0; c->pf_stale = false; c->pf_dirty = false; }

// Counts the windows of every batch that has not been counted yet (all of them behind a stale filter).  Stream-ordered, no host round trip.
int prefilter_count_pending(mdbg_ctx* c) {
    hipStream_t s = c->stream;
    const size_t bytes = prefilter_words(c->pf_n_cells) * sizeof(u32);
    if (c->pf_stale) {
        if (c->pf_cells.p) HIPCHK(c, hipMemsetAsync(c->pf_cells.p, 0, bytes, s));
        c->pf_counted = 0; c->pf_stale = false; c->pf_dirty = true;      // (whatever the table holds was admitted by counts that no longer stand)
    }
    if (c->pf_counted >= c->batches.size()) return MDBG_OK;
    if (!c->pf_cells.p) {                      // first use
        HIPCHK(c, c->pf_cells.ensure(bytes, 0, s));
        HIPCHK(c, hipMemsetAsync(c->pf_cells.p, 0, bytes, s));
    }
    c->res.invalidate(FROM_NODES);
    for (size_t i = c->pf_counted; i < c->batches.size(); ++i) {
        Batch& b = c->batches[i];
        if (b.m1 == b.m0) continue;
        fill_mread_of(c, b);
        launch_prefilter_count(c->pf_cells.as<u32>(), c->pf_n_cells, c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, s);
    }
    c->pf_counted = c->batches.size(); c->pf_dirty = true;
    return MDBG_OK;
}
// In front of an insertion round: every resident batch counted; and when a batch was counted since the last round, windows of batches that are in the table already
// may have become admissible only now — the table is cleared and the round starts from batch 0 (the simple correct rule).
int prefilter_prepare(mdbg_ctx* c) {
    int e = prefilter_count_pending(c); if (e) return e;
    if (c->pf_dirty && c->batches_inserted) { e = clear_table(c); if (e) return e; }
    c->pf_dirty = false;
    return MDBG_OK;
}
// The round's window count in this mode: the admit pass over the batches [first, last) — their admission bits into pf_adm (Batch::adm_word says where), the number of
// admitted windows into SC_BATCHWIN (it sizes the table) and the number of all their windows into SC_NWINDOWS (mdbg_stats.n_windows).
int prefilter_admit(mdbg_ctx* c, size_t first, size_t last) {
    hipStream_t s = c->stream;
    u64 words = 0;
    for (size_t i = first; i < last; ++i) { Batch& b = c->batches[i]; b.adm_word = words; words += (b.m1 - b.m0 + 63) / 64; }
    HIPCHK(c, c->pf_adm.ensure((size_t)(words + 1) * 8, 0, s));
    u64* const admitted = c->shards.as<u64>() + SH_OWNED * CTR_SHARDS;      // (a partitioned context's counter: never partitioned in this mode)
    HIPCHK(c, hipMemsetAsync(admitted, 0, CTR_SHARDS * 8, s));
    HIPCHK(c, hipMemsetAsync(scal(c) + SC_NWINDOWS, 0, 8, s));
    for (size_t i = first; i < last; ++i) {
        Batch& b = c->batches[i];
        if (b.m1 == b.m0) continue;
        fill_mread_of(c, b);
        launch_prefilter_admit(c->pf_cells.as<u32>(), c->pf_n_cells, c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->P.k, c->pf_adm.as<u64>() + b.adm_word, admitted, s);
        launch_count_windows(c->roff.as<u64>(), b.slot0, b.n_reads, c->P.k, scal(c) + SC_NWINDOWS, s);
    }
    launch_sum_shards(admitted, 1, scal(c) + SC_BATCHWIN, s);
    c->batchwin_zero = false;
    return MDBG_OK;
}
}  // namespace
