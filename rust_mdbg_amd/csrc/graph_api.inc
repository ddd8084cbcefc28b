// graph_api.inc — C ABI of the graph stages on the last finalized node table: edges (edges.hip), unitigs (unitigs.hip), tip, bubble and small-component
// removal (simplify.hip), connected components (components.hip), stitched contigs (contigs.hip) and node sequences (node_seqs.hip).  Host code; included by api.inc, whose context, fail() and copy_out() it uses.

// ---- graph edges of the last finalized node table (edges.hip) -------------------------------------------
static int edges_impl(mdbg_ctx* c, float presimp, mdbg_edge_list* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (!(presimp >= 0.0f)) return fail(c, MDBG_E_PARAM, "presimp must be >= 0");
    memset(out, 0, sizeof *out);
    if (!c->nodes_ok && !(c->cap == 0 || c->M == 0)) return fail(c, MDBG_E_STATE, "no finalized node table on this context (call mdbg_finalize / mdbg_finalize_device first)");
    invalidate_results(c, FROM_EDGES); c->last_edges = EdgeResult{};
    if (!c->nodes_ok || c->nodes_n == 0) { c->edges_ok = c->nodes_ok; return MDBG_OK; }
    if (c->nodes_n >= (1ull << 30)) return fail(c, MDBG_E_CAPACITY, "more than 2^30 nodes");
    if (!c->eb) c->eb = edge_buffers_create();
    const FinArgs& F = c->finF;
    EdgeNodes nd; nd.keys = F.o_keys; nd.index = F.o_index; nd.abund = F.o_abund; nd.seqlen = F.o_seqlen; nd.shift = F.o_shift; nd.n = c->nodes_n; nd.k = c->P.k;
    EdgeResult r;
    HIPCHK(c, build_edges(c->eb, nd, presimp, c->stream, &r));
    c->last_edges = r; c->edges_ok = true;
    out->n = r.n; out->presimp_removed = r.presimp_removed;
    if (!to_host) { out->n1 = r.n1; out->o1 = r.o1; out->n2 = r.n2; out->o2 = r.o2; out->overlap = r.overlap; return MDBG_OK; }
    const char* const what = "host copy of the edge list";
    int e;
    if ((e = copy_out(c, c->he_n1, r.n1, r.n, what, &out->n1)) || (e = copy_out(c, c->he_o1, r.o1, r.n, what, &out->o1)) || (e = copy_out(c, c->he_n2, r.n2, r.n, what, &out->n2)) ||
        (e = copy_out(c, c->he_o2, r.o2, r.n, what, &out->o2)) || (e = copy_out(c, c->he_ov, r.overlap, r.n, what, &out->overlap))) return e;
    return MDBG_OK;
}
int mdbg_graph_edges(mdbg_ctx* c, float presimp, mdbg_edge_list* out) { return edges_impl(c, presimp, out, true); }
int mdbg_graph_edges_device(mdbg_ctx* c, float presimp, mdbg_edge_list* out) { return edges_impl(c, presimp, out, false); }

// ---- unitigs + base-space copy plan of the last node table and edge list (unitigs.hip) -------------------
// steps == nullptr: plain compaction (mdbg_graph_unitigs); otherwise the schedule runs first (mdbg_graph_simplify, simplify.hip) and stats is filled
static int unitigs_impl(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats, bool to_host) {
    if (!c || !out || (stats && n_steps && !steps)) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    memset(out, 0, sizeof *out);
    bool with_components = false;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        for (uint32_t i = 0; i < n_steps; ++i) {
            const uint32_t kind = steps[i].kind;
            if (kind != MDBG_SIMPLIFY_TIPS && kind != MDBG_SIMPLIFY_BUBBLES && kind != MDBG_SIMPLIFY_COMPONENTS) return fail(c, MDBG_E_PARAM, "unknown kind of simplification step");
            if (kind == MDBG_SIMPLIFY_COMPONENTS && steps[i].max_nodes == 0 && steps[i].max_bases == 0)
                return fail(c, MDBG_E_PARAM, "a component step without a limit would remove the whole graph");
            with_components |= kind == MDBG_SIMPLIFY_COMPONENTS;
        }
        c->hs_unitigs.assign(n_steps, 0); c->hs_nodes.assign(n_steps, 0);
        stats->n_steps = n_steps; stats->unitigs_removed = c->hs_unitigs.data(); stats->nodes_removed = c->hs_nodes.data();
    }
    invalidate_results(c, FROM_UNITIGS); c->last_ul = UnitigResult{};
    if (c->routed || c->own_world > 1) return fail(c, MDBG_E_STATE, "unitigs are single-GPU only: not available on a routed or partitioned context");
    if (c->cap == 0 || c->M == 0) { c->ulist_ok = true; return MDBG_OK; }      // empty context: empty list
    if (!(c->nodes_ok && c->edges_ok)) return fail(c, MDBG_E_STATE, "no current edge list on this context (call mdbg_finalize* and mdbg_graph_edges* first)");
    if (c->nodes_n == 0) { c->ulist_ok = true; return MDBG_OK; }
    if (!c->ub) c->ub = unitig_buffers_create();
    if (with_components && !c->compb) c->compb = component_buffers_create();
    const FinArgs& F = c->finF;
    UnitigNodes nd; nd.index = F.o_index; nd.abund = F.o_abund; nd.shift_full = F.o_shift_full; nd.src_read = F.o_src_read; nd.src_start = F.o_src_start; nd.src_end = F.o_src_end;
    nd.reversed = F.o_rev; nd.n = c->nodes_n;
    UnitigResult r; int broken = 0;
    SimplifyInfo si{};
    const hipError_t he = stats ? simplify_unitigs(c->ub, c->compb, nd, c->last_edges, steps, n_steps, c->stream, &r, c->hs_unitigs.data(), c->hs_nodes.data(), &si, &broken)
                                : build_unitigs(c->ub, nd, c->last_edges, c->stream, &r, &broken);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "build_unitigs", he);
    if (broken) return fail(c, MDBG_E_DEVICE, "unitig ranking did not settle within ceil(log2(2n)) + 1 rounds, a union-find of a component step ran into its bound, or the walk broke an invariant");
    if (stats) {
        stats->n_compactions = si.n_compactions; stats->n_rounds_total = si.n_rounds_total; stats->n_syncs = si.n_syncs;
        for (uint32_t i = 0; i < n_steps; ++i) { stats->total_unitigs_removed += c->hs_unitigs[i]; stats->total_nodes_removed += c->hs_nodes[i]; }
    }
    c->last_ul = r; c->ulist_ok = true;
    const u64 U = r.n_unitigs, N = r.n_entries, E = r.edges.n;
    out->n_unitigs = U; out->n_entries = N; out->n_rounds = r.n_rounds; out->edges.n = E;
    if (U == 0) return MDBG_OK;                      // a schedule that removed everything: the empty list, as an empty context gives it
    if (!to_host) {
        out->offsets = r.offsets; out->node = r.node; out->ori = r.ori; out->src_read = r.src_read; out->src_begin = r.src_begin; out->len = r.len; out->revcomp = r.revcomp;
        out->dst_offset = r.dst_offset; out->length = r.length; out->kc_sum = r.kc_sum; out->circular = r.circular;
        out->edges.n1 = r.edges.n1; out->edges.o1 = r.edges.o1; out->edges.n2 = r.edges.n2; out->edges.o2 = r.edges.o2; out->edges.overlap = r.edges.overlap;
        return MDBG_OK;
    }
    const char* const what = "host copy of the unitig list";
    int e;
    if ((e = copy_out(c, c->hu_off, r.offsets, U + 1, what, &out->offsets)) || (e = copy_out(c, c->hu_node, r.node, N, what, &out->node)) || (e = copy_out(c, c->hu_ori, r.ori, N, what, &out->ori)) ||
        (e = copy_out(c, c->hu_sread, r.src_read, N, what, &out->src_read)) || (e = copy_out(c, c->hu_sbegin, r.src_begin, N, what, &out->src_begin)) ||
        (e = copy_out(c, c->hu_len, r.len, N, what, &out->len)) || (e = copy_out(c, c->hu_rc, r.revcomp, N, what, &out->revcomp)) || (e = copy_out(c, c->hu_dst, r.dst_offset, N, what, &out->dst_offset)) ||
        (e = copy_out(c, c->hu_length, r.length, U, what, &out->length)) || (e = copy_out(c, c->hu_kc, r.kc_sum, U, what, &out->kc_sum)) || (e = copy_out(c, c->hu_circ, r.circular, U, what, &out->circular)) ||
        (e = copy_out(c, c->hu_n1, r.edges.n1, E, what, &out->edges.n1)) || (e = copy_out(c, c->hu_o1, r.edges.o1, E, what, &out->edges.o1)) || (e = copy_out(c, c->hu_n2, r.edges.n2, E, what, &out->edges.n2)) ||
        (e = copy_out(c, c->hu_o2, r.edges.o2, E, what, &out->edges.o2)) || (e = copy_out(c, c->hu_ov, r.edges.overlap, E, what, &out->edges.overlap))) return e;
    return MDBG_OK;
}
int mdbg_graph_unitigs(mdbg_ctx* c, mdbg_unitig_list* out) { return unitigs_impl(c, nullptr, 0, out, nullptr, true); }
int mdbg_graph_unitigs_device(mdbg_ctx* c, mdbg_unitig_list* out) { return unitigs_impl(c, nullptr, 0, out, nullptr, false); }
int mdbg_graph_simplify(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats) {
    if (!stats) return MDBG_E_PARAM;
    return unitigs_impl(c, steps, n_steps, out, stats, true);
}
int mdbg_graph_simplify_device(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats) {
    if (!stats) return MDBG_E_PARAM;
    return unitigs_impl(c, steps, n_steps, out, stats, false);
}

// ---- connected components of the current unitig list (components.hip) -------------------------------------
static int components_impl(mdbg_ctx* c, mdbg_component_list* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    memset(out, 0, sizeof *out);
    if (c->routed || c->own_world > 1) return fail(c, MDBG_E_STATE, "components are single-GPU only: not available on a routed or partitioned context");
    if (!c->ulist_ok) return fail(c, MDBG_E_STATE, "no current unitig list on this context (call mdbg_graph_unitigs* or mdbg_graph_simplify* first)");
    if (c->last_ul.n_unitigs == 0) return MDBG_OK;
    if (!c->compb) c->compb = component_buffers_create();
    ComponentResult r; int broken = 0;
    const hipError_t he = build_components(c->compb, c->last_ul, c->stream, &r, &broken);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "build_components", he);
    if (broken) return fail(c, MDBG_E_DEVICE, "the union-find of the components ran into its bound of n_unitigs + 1 steps, or an edge names a unitig outside the list");
    const u64 U = r.n_unitigs, K = r.n_components;
    out->n_unitigs = U; out->n_components = K;
    if (!to_host) {
        out->component = r.component; out->first_unitig = r.first_unitig; out->unitigs = r.unitigs; out->nodes = r.nodes; out->bases = r.bases; out->kc_sum = r.kc_sum;
        out->circular = r.circular;
        return MDBG_OK;
    }
    const char* const what = "host copy of the component list";
    int e;
    if ((e = copy_out(c, c->hk_comp, r.component, U, what, &out->component)) || (e = copy_out(c, c->hk_first, r.first_unitig, K, what, &out->first_unitig)) ||
        (e = copy_out(c, c->hk_unitigs, r.unitigs, K, what, &out->unitigs)) || (e = copy_out(c, c->hk_nodes, r.nodes, K, what, &out->nodes)) ||
        (e = copy_out(c, c->hk_bases, r.bases, K, what, &out->bases)) || (e = copy_out(c, c->hk_kc, r.kc_sum, K, what, &out->kc_sum)) ||
        (e = copy_out(c, c->hk_circ, r.circular, K, what, &out->circular))) return e;
    return MDBG_OK;
}
int mdbg_graph_components(mdbg_ctx* c, mdbg_component_list* out) { return components_impl(c, out, true); }
int mdbg_graph_components_device(mdbg_ctx* c, mdbg_component_list* out) { return components_impl(c, out, false); }

// ---- contigs stitched on the GPU from the resident read store (contigs.hip) ------------------------------
int mdbg_kept_reads(mdbg_ctx* c, uint64_t* n_reads, uint64_t* n_bases, uint64_t* bytes) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    u64 r = 0, b = 0, y = 0;
    for (const Batch& bt : c->batches) if (bt.kept) { r += bt.kept->n_reads; b += bt.kept->n_bases; y += bt.kept->bytes(); }
    if (n_reads) *n_reads = r;
    if (n_bases) *n_bases = b;
    if (bytes) *bytes = y;
    return MDBG_OK;
}
// the resident read store as the gather kernels take it: one descriptor per batch, sorted by first ordinal
static int kept_table(mdbg_ctx* c, std::vector<KeptDesc>& tab) {
    for (const Batch& b : c->batches) {
        if (!b.kept) return fail(c, MDBG_E_STATE, "a resident batch came without bases (an imported sketch): its reads are not kept");
        const KeptReads& k = *b.kept;
        KeptDesc d{}; d.first_ordinal = b.first_ordinal; d.n_reads = k.n_reads; d.planes = k.planes(); d.n_words = k.n_words; d.offsets = k.offsets();
        d.exc_pos = k.n_exc ? k.exc_pos() : nullptr; d.exc_val = k.n_exc ? k.exc_val() : nullptr; d.n_exc = k.n_exc;
        tab.push_back(d);
    }
    std::sort(tab.begin(), tab.end(), [](const KeptDesc& a, const KeptDesc& b) { return a.first_ordinal < b.first_ordinal; });
    if (tab.size() >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many kept batches");
    return MDBG_OK;
}
static int contigs_impl(mdbg_ctx* c, uint64_t min_len, mdbg_contig_seqs* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    memset(out, 0, sizeof *out);
    if (!(c->P.flags & MDBG_FLAG_KEEP_READS)) return fail(c, MDBG_E_STATE, "the context does not keep its reads (create it with MDBG_FLAG_KEEP_READS)");
    if (c->routed || c->own_world > 1) return fail(c, MDBG_E_STATE, "contigs are single-GPU only: not available on a routed or partitioned context");
    if (!c->ulist_ok) return fail(c, MDBG_E_STATE, "no current unitig list on this context (call mdbg_graph_unitigs* or mdbg_graph_simplify* first)");
    std::vector<KeptDesc> tab;
    { const int e = kept_table(c, tab); if (e) return e; }
    if (!c->cb) c->cb = contig_buffers_create();
    ContigResult r;
    const hipError_t he = stitch_contigs(c->cb, c->last_ul, tab.data(), (u32)tab.size(), min_len, c->stream, &r);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "stitch_contigs", he);
    c->ms_stitch = r.ms_stitch;
    if (r.err & 1u) return fail(c, MDBG_E_STATE, "an entry of the copy plan names a read that is not kept");
    if (r.err & 2u) return fail(c, MDBG_E_PARAM, "an entry of the copy plan lies outside its read (not the reads the table was built from)");
    out->n_contigs = r.n_contigs; out->n_bases = r.n_bases;
    if (!to_host) { out->bases = r.bases; out->offsets = r.offsets; out->unitig = r.unitig; return MDBG_OK; }
    const char* const what = "host copy of the contigs";
    int e;
    if ((e = copy_out(c, c->hc_bases, r.bases, r.n_bases, what, &out->bases)) || (e = copy_out(c, c->hc_off, r.offsets, r.n_contigs + 1, what, &out->offsets)) ||      // (offsets: never empty)
        (e = copy_out(c, c->hc_unitig, r.unitig, r.n_contigs, what, &out->unitig))) return e;
    return MDBG_OK;
}
int mdbg_graph_contigs(mdbg_ctx* c, uint64_t min_len, mdbg_contig_seqs* out) { return contigs_impl(c, min_len, out, true); }
int mdbg_graph_contigs_device(mdbg_ctx* c, uint64_t min_len, mdbg_contig_seqs* out) { return contigs_impl(c, min_len, out, false); }
int mdbg_contigs_ms(mdbg_ctx* c, double* ms) {
    if (!c || !ms) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    *ms = c->ms_stitch;
    return MDBG_OK;
}

// ---- the node table's sequences gathered on the GPU from the resident read store, in bounded chunks (node_seqs.hip) ----
static int node_seqs_impl(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    memset(out, 0, sizeof *out);
    out->first_row = first_row;
    if (!(c->P.flags & MDBG_FLAG_KEEP_READS)) return fail(c, MDBG_E_STATE, "the context does not keep its reads (create it with MDBG_FLAG_KEEP_READS)");
    if (c->routed || c->own_world > 1) return fail(c, MDBG_E_STATE, "node sequences are single-GPU only: not available on a routed or partitioned context");
    if (!c->nodes_ok && !c->nodes_none)
        return fail(c, MDBG_E_STATE, "no finalized node table on this context (call mdbg_finalize* first; an ingest, rewind or reset call ends the table)");
    std::vector<KeptDesc> tab;
    { const int e = kept_table(c, tab); if (e) return e; }
    if (!c->nsb) c->nsb = node_seq_buffers_create();
    const FinArgs& F = c->finF;
    NodeSeqRows rows; rows.src_read = F.o_src_read; rows.src_start = F.o_src_start; rows.src_end = F.o_src_end; rows.reversed = F.o_rev; rows.n = c->nodes_ok ? c->nodes_n : 0;      // (nodes_none: the finalize of an empty context, no rows)
    hipError_t he;
    if (!c->nseq_prefix_ok && rows.n) {              // once per node table
        he = node_seq_prefix(c->nsb, rows, c->stream);
        if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "node_seq_prefix", he);
        c->nseq_prefix_ok = true;
    }
    NodeSeqResult r;
    he = node_seq_chunk(c->nsb, rows, tab.data(), (u32)tab.size(), first_row, max_rows, max_bases, c->stream, &r);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "node_seq_chunk", he);
    c->ms_node_seqs = r.ms_gather;
    if (r.err & 1u) return fail(c, MDBG_E_STATE, "a row of the node table names a read that is not kept");
    if (r.err & 2u) return fail(c, MDBG_E_PARAM, "a row of the node table lies outside its read (not the reads the table was built from)");
    out->n_rows = r.n_rows; out->n_bases = r.n_bases;
    if (!to_host) { out->bases = r.bases; out->offsets = r.offsets; return MDBG_OK; }
    const char* const what = "host copy of the node sequences";
    int e;
    if ((e = copy_out(c, c->hn_bases, r.bases, r.n_bases, what, &out->bases)) || (e = copy_out(c, c->hn_off, r.offsets, r.n_rows + 1, what, &out->offsets))) return e;      // (offsets: never empty)
    return MDBG_OK;
}
int mdbg_graph_node_seqs(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out) { return node_seqs_impl(c, first_row, max_rows, max_bases, out, true); }
int mdbg_graph_node_seqs_device(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out) { return node_seqs_impl(c, first_row, max_rows, max_bases, out, false); }
int mdbg_node_seqs_ms(mdbg_ctx* c, double* ms) {
    if (!c || !ms) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    *ms = c->ms_node_seqs;
    return MDBG_OK;
}

// ---- the resident reads threaded through the current unitig list (place_windows.hip, read_paths.hip) ---------
// roff[r] where the host knows it without asking the device: r is the first slot of a batch, or one past its last
static bool known_read_offset(const mdbg_ctx* c, u64 r, u64* v) {
    for (const Batch& b : c->batches) {
        if (b.slot0 == r) { *v = b.m0; return true; }
        if ((u64)b.slot0 + b.n_reads == r) { *v = b.m1; return true; }
    }
    return false;
}
static int read_paths_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out, bool to_host) {
    if (!c || !out) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    memset(out, 0, sizeof *out);
    out->first_read = first_read;
    c->ms_read_paths = 0;
    if (c->routed || c->own_world > 1) return fail(c, MDBG_E_STATE, "read paths are single-GPU only: not available on a routed or partitioned context");
    if (!c->ulist_ok) return fail(c, MDBG_E_STATE, "no current unitig list on this context (call mdbg_graph_unitigs* or mdbg_graph_simplify* first)");
    if (!c->nodes_ok && !(c->cap == 0 || c->M == 0)) return fail(c, MDBG_E_STATE, "the node table the unitig list was built from is not current");
    const UnitigResult& ul = c->last_ul;
    if (ul.n_unitigs == 0 || first_read >= c->n_slots) return MDBG_OK;      // an empty context, an empty list, a range behind the store
    if (ul.n_entries >= (1ull << 30) || c->nodes_n >= (1ull << 30)) return fail(c, MDBG_E_CAPACITY, "more than 2^30 nodes");
    hipStream_t s = c->stream;
    const u64 r0 = first_read, r1 = max_reads && max_reads < c->n_slots - r0 ? r0 + max_reads : c->n_slots;
    ReadPathRange rg{};
    const bool known0 = known_read_offset(c, r0, &rg.i0), known1 = known_read_offset(c, r1, &rg.i1);
    if (!known0) HIPCHK(c, hipMemcpyAsync(&rg.i0, c->roff.as<u64>() + r0, 8, hipMemcpyDeviceToHost, s));
    if (!known1) HIPCHK(c, hipMemcpyAsync(&rg.i1, c->roff.as<u64>() + r1, 8, hipMemcpyDeviceToHost, s));
    if (!(known0 && known1)) HIPCHK(c, hipStreamSynchronize(s));      // (a range that starts or ends inside a batch: one more wait, for its two offsets)
    if (rg.i1 < rg.i0 || rg.i1 > c->M) return fail(c, MDBG_E_DEVICE, "the read offsets of the store are not ascending");
    if (rg.i1 - rg.i0 >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers in the range of reads");
    for (Batch& b : c->batches) fill_mread_of(c, b);
    FinArgs F = c->finF;
    F.mh = c->mh.as<u64>(); F.roff = c->roff.as<u64>(); F.mread = c->mread.as<u32>();
    rg.roff = F.roff; rg.mread = F.mread; rg.first_read = (u32)r0; rg.n_reads = (u32)(r1 - r0); rg.k = c->P.k;
    rg.by_slot0 = F.bt.by_slot0; rg.by_slot_first = F.bt.by_slot_first; rg.n_batches = F.bt.n;
    if (!c->rpb) c->rpb = read_path_buffers_create();
    ReadPathPlan plan;
    hipError_t he = read_paths_begin(c->rpb, ul, F.o_index, c->nodes_n, rg, s, &plan);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "read_paths_begin", he);
    launch_place_windows(table_args(c), F, c->fin_words, plan, F.mh, F.mread, F.roff, rg.i0, rg.i1, s);
    ReadPathResult r;
    he = read_paths_end(c->rpb, ul, rg, s, &r);
    if (he != hipSuccess) return fail(c, he == hipErrorOutOfMemory ? MDBG_E_NOMEM : MDBG_E_DEVICE, "read_paths_end", he);
    c->ms_read_paths = r.ms;
    if (r.defect & RP_DEFECT_ENTRY) return fail(c, MDBG_E_DEVICE, "an entry of the unitig list names a node index that is not a row of the node table");
    if (r.defect & RP_DEFECT_PROBE) return fail(c, MDBG_E_DEVICE, "a probe sequence of the read paths visited every slot of the table");
    if (r.defect) return fail(c, MDBG_E_DEVICE, "a solid slot's first sighting is no row of the node table");
    const u64 nr = r.n_reads, ns = r.n_steps, U = r.n_unitigs;
    out->n_reads = nr; out->n_windows = r.n_windows; out->n_placed = r.n_placed; out->n_steps = ns; out->n_unitigs = U;
    if (!to_host) {
        out->ordinal = r.ordinal; out->read_windows = r.read_windows; out->step_offsets = r.step_offsets; out->first_window = r.first_window; out->step_windows = r.step_windows; out->unitig = r.unitig;
        out->first_entry = r.first_entry; out->strand = r.strand; out->support_windows = r.support_windows; out->support_steps = r.support_steps;
        return MDBG_OK;
    }
    const char* const what = "host copy of the read paths";
    int e;
    if ((e = copy_out(c, c->hr_ord, r.ordinal, nr, what, &out->ordinal)) || (e = copy_out(c, c->hr_rw, r.read_windows, nr, what, &out->read_windows)) || (e = copy_out(c, c->hr_off, r.step_offsets, nr + 1, what, &out->step_offsets)) ||
        (e = copy_out(c, c->hr_fw, r.first_window, ns, what, &out->first_window)) || (e = copy_out(c, c->hr_nw, r.step_windows, ns, what, &out->step_windows)) ||
        (e = copy_out(c, c->hr_unitig, r.unitig, ns, what, &out->unitig)) || (e = copy_out(c, c->hr_fe, r.first_entry, ns, what, &out->first_entry)) ||
        (e = copy_out(c, c->hr_strand, r.strand, ns, what, &out->strand)) || (e = copy_out(c, c->hr_supw, r.support_windows, U, what, &out->support_windows)) ||
        (e = copy_out(c, c->hr_sups, r.support_steps, U, what, &out->support_steps))) return e;
    return MDBG_OK;
}
int mdbg_graph_read_paths(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out) { return read_paths_impl(c, first_read, max_reads, out, true); }
int mdbg_graph_read_paths_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out) { return read_paths_impl(c, first_read, max_reads, out, false); }
int mdbg_read_paths_ms(mdbg_ctx* c, double* ms) {
    if (!c || !ms) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    *ms = c->ms_read_paths;
    return MDBG_OK;
}
