// finalize_api.inc — the node table of the resident windows: mdbg_finalize*, the two-phase finalize of a partitioned table, mdbg_nodes_digest.  Included inside api.inc's extern "C".
// FinArgs shared by finalize and the resolve_* entry points: batch table (sorted by first ordinal -> dense order of
// the ordinals), zeroed bitmaps over the resident minimizers, prefix buffers
static int fin_setup(mdbg_ctx* c, FinArgs& F, u64& n_words_out, bool byte_maps = false) {
    hipStream_t s = c->stream;
    c->res.invalidate(FROM_NODES);
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
                // A claim-map finalize MOVES marks (fin_mark_claims_kernel: off the claimer, onto the first sighting it sees) and clears only the claimer's byte the next
                // time.  That holds as long as first sightings stay where they are: a batch that arrives afterwards BELOW the largest first ordinal that finalize saw may
                // hold an earlier sighting of a key whose mark has been moved, and the mark on the sighting in between would stay (the key counted twice, every row behind it
                // shifted).  From such a batch on the table is finalized through the zeroed byte maps, until it is cleared.  Host-side and by ordinals alone, so the same
                // rule covers a partitioned table (own_world > 1), whose peers' batches are registered here like its own.
                if (c->claims_ok && c->claims_fin_batches)
                    for (size_t i = c->claims_fin_batches; i < c->batches.size(); ++i)
                        if (c->batches[i].first_ordinal < c->claims_fin_top) { c->claims_ok = false; break; }
                const bool use_claims = c->claims_ok && !c->routed && c->claim.p && c->batches_inserted == c->batches.size() && getenv("MDBG_NO_CLAIMS") == nullptr;
                bool dense_is_store = c->own_world <= 1 && acc == c->M;
                for (u32 i = 0; i < nb && dense_is_store; ++i) dense_is_store = !bs[i].partial && rb[i] == bs[i].m0;
                if (use_claims) {
                    F.claims = dense_is_store ? 1 : 2;
                    c->claims_fin_batches = c->batches.size(); c->claims_fin_top = nb ? fo[nb - 1] : 0;      // (what this finalize's marks rest on, see above)
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
// j* = A + 65536 * floor((count - A) / 65536) instead of the A-th (finalize.hip, wrap_list_kernel).  n_bound: upper bound of
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
    HIPCHK(c, sort_segments_u64(c->res.edges.buf.get(), c->w_occ.as<u64>(), c->w_sorted.as<u64>(), total, (u32)n_w, c->w_start.as<u32>(), s));
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
// The node rows' block: fin_out sized for `rows` rows, every column rounded up to 256 bytes, and F.o_* set to the ten columns; row_column: room for a partition's
// global rows (F.o_row) between src_end and index as well.
static int carve_node_rows(mdbg_ctx* c, FinArgs& F, size_t rows, bool row_column) {
    size_t off = 0; auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_keys = carve(rows * c->P.k * 8), o_sf = carve(rows * 16), o_sr = carve(rows * 8), o_ss = carve(rows * 8), o_se = carve(rows * 8), o_row = row_column ? carve(rows * 8) : 0,
                 o_idx = carve(rows * 4), o_sl = carve(rows * 4), o_ab = carve(rows * 2), o_sh = carve(rows * 4), o_rv = carve(rows);
    HIPCHK(c, c->fin_out.ensure(off + 256, 0, c->stream));
    u8* fo_ = c->fin_out.as<u8>();
    F.o_keys = (u64*)(fo_ + o_keys); F.o_shift_full = (u64*)(fo_ + o_sf); F.o_src_read = (u64*)(fo_ + o_sr); F.o_src_start = (u64*)(fo_ + o_ss);
    F.o_src_end = (u64*)(fo_ + o_se); F.o_index = (u32*)(fo_ + o_idx); F.o_seqlen = (u32*)(fo_ + o_sl); F.o_abund = (u16*)(fo_ + o_ab);
    F.o_shift = (u16*)(fo_ + o_sh); F.o_rev = fo_ + o_rv; F.o_row = row_column ? (u64*)(fo_ + o_row) : nullptr;
    return MDBG_OK;
}
// the rows are on the device (c->finF.o_*): hand them over as device pointers, copied into the context's host columns, or (mdbg_finalize_gfa) only the three columns
// an S line prints copied and the others left null
enum NodesTo { TO_DEVICE, TO_HOST, TO_HOST_GFA };
static int finalize_hand_over(mdbg_ctx* c, mdbg_nodes* out, NodesTo to, u64 n) {
    const FinArgs& F = c->finF;
    auto& H = c->res.nodes;
    const bool all = to != TO_HOST_GFA;
    HandOver ho{c, "host copy of the node table", to != TO_DEVICE};
    if (all) ho.col(F.o_keys, n * c->P.k, H.keys, &out->keys);
    ho.col(F.o_index, n, H.index, &out->index);
    ho.col(F.o_abund, n, H.abund, &out->abundance);
    ho.col(F.o_seqlen, n, H.seqlen, &out->seqlen);
    if (!all) return ho.err;
    ho.col(F.o_shift, 2 * n, H.shift, &out->shift);
    ho.col(F.o_shift_full, 2 * n, H.shift_full, &out->shift_full);
    ho.col(F.o_src_read, n, H.src_read, &out->src_read);
    ho.col(F.o_src_start, n, H.src_start, &out->src_start);
    ho.col(F.o_src_end, n, H.src_end, &out->src_end);
    ho.col(F.o_rev, n, H.rev, &out->reversed);
    return ho.err;
}
// finalize, phase 2: ranks from the (possibly all-reduced) bitmaps, then the node rows of this context's solid keys.
// partitioned: rows are written compactly in list order and their global row goes to *d_row.
static int finalize_end_impl(mdbg_ctx* c, mdbg_nodes* out, NodesTo to, bool partitioned, const uint64_t** d_row, uint64_t* n_solid_global, bool fused = false) {
    hipStream_t s = c->stream;
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
        e = carve_node_rows(c, F, cap_rows, false); if (e) return e;      // (no room for global rows: this path is never partitioned)
        HIPCHK(c, c->fin_order.ensure(cap_rows * 8, 0, s));
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
            c->res.node_table_is(NodeTable::ROWS, n_solid);
            return finalize_hand_over(c, out, to, n_solid);
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
    e = carve_node_rows(c, F, n, true); if (e) return e;
    if (!partitioned) F.o_row = nullptr;
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
    c->res.node_table_is(partitioned ? NodeTable::NONE : NodeTable::ROWS, n_solid);
    return finalize_hand_over(c, out, to, n);
}

static int finalize_impl(mdbg_ctx* c, mdbg_nodes* out, NodesTo to) {
    MDBG_ENTER(c, out);
    if (c->routed) return fail(c, MDBG_E_STATE, "a routed table is finalized by the distributed driver (mdbg_routed_export / mdbg_resolve_* / mdbg_routed_keys)");
    memset(out, 0, sizeof *out);
    out->k = c->P.k;
    if (prefilter_on(c)) { const int pe = insert_resident_impl(c); if (pe) return pe; }      // the admitted windows of everything resident, inserted now (the ingest calls only count)
    if (nothing_resident(c)) { c->res.node_table_is(NodeTable::EMPTY, 0); return MDBG_OK; }
    int e = finalize_begin_impl(c, true); if (e) return e;
    return finalize_end_impl(c, out, to, false, nullptr, nullptr, true);
}
int mdbg_finalize(mdbg_ctx* c, mdbg_nodes* out) { return finalize_impl(c, out, TO_HOST); }
int mdbg_finalize_device(mdbg_ctx* c, mdbg_nodes* out) { return finalize_impl(c, out, TO_DEVICE); }
int mdbg_finalize_gfa(mdbg_ctx* c, mdbg_nodes* out) { return finalize_impl(c, out, TO_HOST_GFA); }

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

int mdbg_finalize_begin(mdbg_ctx* c, uint64_t** d_bm_first, uint64_t** d_bm_solid, uint64_t* n_words) {
    MDBG_ENTER(c, d_bm_first && d_bm_solid && n_words);
    if (c->routed) return fail(c, MDBG_E_STATE, "not available for a routed table");
    if (prefilter_on(c)) { const int pe = insert_resident_impl(c); if (pe) return pe; }
    if (!c->M) {                       // no minimizer anywhere (empty input, or every read shorter than l): an empty table, not an error
        c->fin_open = true; c->fin_words = 0;      // (nothing resident: no node table can be current, M == 0 since the last clear_table)
        *d_bm_first = nullptr; *d_bm_solid = nullptr; *n_words = 0;
        return MDBG_OK;
    }
    if (!c->cap) { int e0 = table_reserve(c, 0); if (e0) return e0; }
    int e = finalize_begin_impl(c, false); if (e) return e;
    *d_bm_first = c->bm_first.as<u64>(); *d_bm_solid = c->bm_solid.as<u64>(); *n_words = c->fin_words;
    return MDBG_OK;
}

int mdbg_finalize_end(mdbg_ctx* c, mdbg_nodes* out, const uint64_t** d_row, uint64_t* n_nodes_global) {
    MDBG_ENTER(c, out);
    if (!c->fin_open) return fail(c, MDBG_E_STATE, "mdbg_finalize_begin was not called");
    memset(out, 0, sizeof *out);
    out->k = c->P.k;
    if (!c->fin_words) {               // see mdbg_finalize_begin: nothing resident
        c->fin_open = false;
        if (d_row) *d_row = nullptr;
        if (n_nodes_global) *n_nodes_global = 0;
        return MDBG_OK;
    }
    return finalize_end_impl(c, out, TO_DEVICE, true, d_row, n_nodes_global);
}
