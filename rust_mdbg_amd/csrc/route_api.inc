// route_api.inc — C ABI of the multi-GPU stage (routing, owner-side insertion, cross-rank resolution)
extern "C" {

int mdbg_route_pack(mdbg_ctx* c, uint32_t world, const uint64_t** d_records, uint64_t* counts) {
    if (!c || !counts || !d_records) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (prefilter_on(c)) return fail(c, MDBG_E_STATE, PF_UNAVAILABLE);
    if (world < 1 || world > 64) return fail(c, MDBG_E_PARAM, "world must be 1..64");
    hipStream_t s = c->stream;
    const u32 k = c->P.k, RS = k + 2;
    // block layout over all pending batches
    u32 n_blocks = 0;
    for (size_t b = c->batches_inserted; b < c->batches.size(); ++b) n_blocks += route_blocks(c->batches[b].m0, c->batches[b].m1);
    HIPCHK(c, c->route_tmp.ensure((size_t)n_blocks * world * (4 + 8) + 64 * 16 + 256, 0, s));
    HIPCHK(c, c->route_h.ensure((c->M + 1) * 8, 0, s));
    HIPCHK(c, c->route_f.ensure(c->M + 16, 0, s));
    u64* d_tot = c->route_tmp.as<u64>();                  // [64] bucket sizes
    u64* d_base = d_tot + 64;                             // [64] bucket bases
    u64* d_off = d_base + 64;                             // [n_blocks][world]
    u32* d_cnt = (u32*)(d_off + (size_t)n_blocks * world);    // [n_blocks][world]
    STAGE_EVENT(c, c->ev0, s);
    RouteArgs a{};
    a.mh = c->mh.as<u64>(); a.mread = c->mread.as<u32>(); a.roff = c->roff.as<u64>(); a.k = k; a.world = world;
    a.hbuf = c->route_h.as<u64>(); a.wflag = c->route_f.as<u8>(); a.blk_cnt = d_cnt; a.blk_off = d_off; a.out = nullptr;
    u32 blk = 0;
    for (size_t b = c->batches_inserted; b < c->batches.size(); ++b) {
        const Batch& B = c->batches[b];
        a.i0 = B.m0; a.i1 = B.m1; a.slot0 = B.slot0; a.first_ordinal = B.first_ordinal; a.blk0 = blk;
        launch_route_count(a, s);
        blk += route_blocks(B.m0, B.m1);
    }
    u64 h_tot[64]; memset(h_tot, 0, sizeof h_tot);
    if (n_blocks) {
        launch_route_scan(d_cnt, n_blocks, world, d_off, d_tot, s);
        HIPCHK(c, hipMemcpyAsync(h_tot, d_tot, world * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    u64 total = 0, base[64];
    for (u32 d = 0; d < 64; ++d) { base[d] = total; if (d < world) { counts[d] = h_tot[d]; total += h_tot[d]; } }
    HIPCHK(c, c->route_out.ensure((total * RS + 2) * 8, 0, s));
    HIPCHK(c, hipMemcpyAsync(d_base, base, 64 * 8, hipMemcpyHostToDevice, s));
    a.out = c->route_out.as<u64>();
    blk = 0;
    for (size_t b = c->batches_inserted; b < c->batches.size(); ++b) {
        const Batch& B = c->batches[b];
        a.i0 = B.m0; a.i1 = B.m1; a.slot0 = B.slot0; a.first_ordinal = B.first_ordinal; a.blk0 = blk;
        launch_route_write(a, d_base, s);
        blk += route_blocks(B.m0, B.m1);
    }
    STAGE_EVENT(c, c->ev1, s);
    HIPCHK(c, hipStreamSynchronize(s));
    c->ms_insert += ev_ms(c);
    c->batches_inserted = c->batches.size();
    c->n_windows += total;
    *d_records = c->route_out.as<u64>();
    return MDBG_OK;
}

int mdbg_arena_reserve(mdbg_ctx* c, uint64_t n, uint64_t** d_tail) {
    if (!c || !d_tail) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->n_records + n >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 routed records on one device");
    const u64 RS = (u64)c->P.k + 2;
    HIPCHK(c, c->arena.ensure((c->n_records + n) * RS * 8 + 64, c->n_records * RS * 8, c->stream));
    *d_tail = c->arena.as<u64>() + c->n_records * RS;
    return MDBG_OK;
}

int mdbg_insert_records(mdbg_ctx* c, const uint64_t* d_records, uint64_t n) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (prefilter_on(c)) return fail(c, MDBG_E_STATE, PF_UNAVAILABLE);
    if (!c->routed && c->n_distinct) return fail(c, MDBG_E_STATE, "table already holds locally inserted k-min-mers");
    c->routed = true;
    if (!n) return MDBG_OK;
    if (!d_records) return fail(c, MDBG_E_PARAM, "null records");
    hipStream_t s = c->stream;
    const u64 RS = (u64)c->P.k + 2;
    uint64_t* tail = nullptr;
    int e = mdbg_arena_reserve(c, n, &tail); if (e) return e;
    if (d_records != tail)                                 // not received in place: copy into the arena
        HIPCHK(c, hipMemcpyAsync(tail, d_records, n * RS * 8, hipMemcpyDeviceToDevice, s));
    u64 sc[SC_N];
    e = read_scalars(c, sc); if (e) return e;
    c->n_distinct = sc[SC_NDISTINCT];
    e = table_reserve(c, n); if (e) return e;
    STAGE_EVENT(c, c->ev0, s);
    launch_insert_records(table_args(c), c->n_records, c->n_records + n, scal(c) + SC_NWINDOWS, s);
    STAGE_EVENT(c, c->ev1, s);
    e = read_scalars(c, sc); if (e) return e;
    c->ms_insert += ev_ms(c);
    c->n_distinct = sc[SC_NDISTINCT];
    c->n_records += n;
    return MDBG_OK;
}

int mdbg_routed_export(mdbg_ctx* c, uint32_t world, const uint64_t* span_lo, const uint32_t* span_rank, uint32_t n_spans, mdbg_routed_lists* out) {
    if (!c || !out || !span_lo || !span_rank) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (prefilter_on(c)) return fail(c, MDBG_E_STATE, PF_UNAVAILABLE);
    if (world < 1 || world > 64 || n_spans < 1 || n_spans > 4096) return fail(c, MDBG_E_PARAM, "bad world / spans");
    memset(out, 0, sizeof *out);
    hipStream_t s = c->stream;
    u64 sc[SC_N];
    int e = read_scalars(c, sc); if (e) return e;
    const u64 nd = c->cap ? sc[SC_NDISTINCT] : 0;
    if (!nd) return MDBG_OK;
    c->n_distinct = nd;
    ExportArgs a{}; u64 n_words = 0;
    e = fin_setup(c, a.F, n_words); if (e) return e;
    const u32 W2 = 2 * world;
    const u32 nb = (u32)((c->cap + 1023) / 1024);
    // scratch: spans | bucket sizes | bucket bases | per-block offsets | per-block counts
    const size_t span_bytes = ((size_t)n_spans * 12 + 15) & ~(size_t)15;
    HIPCHK(c, c->route_tmp.ensure(span_bytes + 128 * 16 + (size_t)nb * W2 * 12 + 256, 0, s));
    u8* base = c->route_tmp.as<u8>();
    u64* d_span_lo = (u64*)base; u32* d_span_rank = (u32*)(base + (size_t)n_spans * 8);
    u64* d_tot = (u64*)(base + span_bytes); u64* d_base = d_tot + 128; u64* d_off = d_base + 128; u32* d_cnt = (u32*)(d_off + (size_t)nb * W2);
    HIPCHK(c, hipMemcpyAsync(d_span_lo, span_lo, (size_t)n_spans * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_span_rank, span_rank, (size_t)n_spans * 4, hipMemcpyHostToDevice, s));
    // outputs, one allocation: a_first[nd] s_ath[nd] s_slot[nd] s_idx1[nd] s_count[nd] a_solid[nd]
    HIPCHK(c, c->fin_out.ensure(nd * 37 + 4096, 0, s));
    a.a_first = c->fin_out.as<u64>(); a.s_ath = a.a_first + nd; a.s_slot = a.s_ath + nd; a.s_idx1 = a.s_slot + nd;
    a.s_count = (u32*)(a.s_idx1 + nd); a.a_solid = (u8*)(a.s_count + nd);
    a.span_lo = d_span_lo; a.span_rank = d_span_rank; a.n_spans = n_spans; a.world = world;
    a.blk_cnt = d_cnt; a.blk_off = d_off; a.bucket_base = d_base;
    if (c->P.min_abundance > MDBG_CASCADE_MAX) { if (c->n_distinct) { e = resolve_wrapped(c, a.F, c->n_distinct, true); if (e) return e; } }
    else if (c->n_records >= 65536) { e = resolve_wrapped(c, a.F, c->n_records / 65536 + 1, true); if (e) return e; }
    STAGE_EVENT(c, c->ev0, s);
    launch_export_grouped(a, false, s);
    launch_route_scan(d_cnt, nb, W2, d_off, d_tot, s);
    u64 h_tot[128];
    HIPCHK(c, hipMemcpyAsync(h_tot, d_tot, W2 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    u64 hb[128]; u64 accA = 0, accS = 0;
    for (u32 d = 0; d < world; ++d) { hb[d] = accA; out->counts_all[d] = h_tot[d]; accA += h_tot[d]; }
    for (u32 d = 0; d < world; ++d) { hb[world + d] = accS; out->counts_solid[d] = h_tot[world + d]; accS += h_tot[world + d]; }
    HIPCHK(c, hipMemcpyAsync(d_base, hb, W2 * 8, hipMemcpyHostToDevice, s));
    launch_export_grouped(a, true, s);
    STAGE_EVENT(c, c->ev1, s);
    HIPCHK(c, hipStreamSynchronize(s));
    c->ms_finalize += ev_ms(c);
    out->n_all = accA; out->n_solid = accS;
    out->d_first = a.a_first; out->d_solid = a.a_solid; out->d_ath = a.s_ath; out->d_slot = a.s_slot; out->d_count = a.s_count; out->d_idx_all = a.s_idx1;
    return MDBG_OK;
}

int mdbg_resolve_first(mdbg_ctx* c, const uint64_t* d_ord, const uint8_t* d_solid, uint64_t n, uint64_t* d_rank_first, uint64_t* d_rank_solid,
                       uint64_t* total_first, uint64_t* total_solid) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (total_first) *total_first = 0;
    if (total_solid) *total_solid = 0;
    if (!n) return MDBG_OK;
    if (!d_ord || !d_solid || !d_rank_first || !d_rank_solid) return fail(c, MDBG_E_PARAM, "null buffer");
    if (!c->M || c->batches.empty()) return fail(c, MDBG_E_STATE, "no resident sketches to resolve ordinals against");
    hipStream_t s = c->stream;
    FinArgs F{}; u64 n_words = 0;
    int e = fin_setup(c, F, n_words); if (e) return e;
    STAGE_EVENT(c, c->ev0, s);
    launch_resolve_mark(F, d_ord, d_solid, n, s);
    launch_popc_prefix2(F.bm_first, F.bm_solid, n_words, c->popc_tmp.as<u32>(), c->pre_first.as<u32>(), c->pre_solid.as<u32>(), s);
    launch_resolve_rank(F, d_ord, n, d_rank_first, d_rank_solid, s);
    STAGE_EVENT(c, c->ev1, s);
    // totals = popcount of the whole bitmaps = prefix of the last word + its popcount
    u32 lastpre[2]; u64 lastw[2];
    HIPCHK(c, hipMemcpyAsync(&lastpre[0], c->pre_first.as<u32>() + (n_words - 1), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&lastpre[1], c->pre_solid.as<u32>() + (n_words - 1), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&lastw[0], c->bm_first.as<u64>() + (n_words - 1), 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&lastw[1], c->bm_solid.as<u64>() + (n_words - 1), 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->ms_finalize += ev_ms(c);
    if (total_first) *total_first = (u64)lastpre[0] + (u64)__builtin_popcountll(lastw[0]);
    if (total_solid) *total_solid = (u64)lastpre[1] + (u64)__builtin_popcountll(lastw[1]);
    return MDBG_OK;
}

int mdbg_resolve_meta(mdbg_ctx* c, const uint64_t* d_ord, uint64_t n, uint64_t* d_meta) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!n) return MDBG_OK;
    if (!d_ord || !d_meta) return fail(c, MDBG_E_PARAM, "null buffer");
    if (!c->M || c->batches.empty()) return fail(c, MDBG_E_STATE, "no resident sketches to resolve ordinals against");
    hipStream_t s = c->stream;
    FinArgs F{}; u64 n_words = 0;
    int e = fin_setup(c, F, n_words); if (e) return e;
    STAGE_EVENT(c, c->ev0, s);
    launch_resolve_meta(F, d_ord, n, d_meta, s);
    STAGE_EVENT(c, c->ev1, s);
    HIPCHK(c, hipStreamSynchronize(s));
    c->ms_finalize += ev_ms(c);
    return MDBG_OK;
}

int mdbg_routed_keys(mdbg_ctx* c, const uint64_t* d_slot, uint64_t n, uint64_t* d_keys) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!n) return MDBG_OK;
    if (!d_slot || !d_keys) return fail(c, MDBG_E_PARAM, "null buffer");
    if (!c->cap) return fail(c, MDBG_E_STATE, "empty table");
    hipStream_t s = c->stream;
    launch_slot_keys(c->tab.as<Slot>(), table_args(c).ks, d_slot, n, d_keys, s);
    HIPCHK(c, hipStreamSynchronize(s));
    return MDBG_OK;
}

}  // extern "C"
