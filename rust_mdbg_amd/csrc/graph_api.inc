// graph_api.inc — C ABI of the graph stages on the last finalized node table: edges (edges.hip), unitigs (unitigs.hip), tip, bubble and small-component
// removal (simplify.hip), connected components (components.hip), stitched contigs (contigs.hip), node sequences (node_seqs.hip), and the stages that
// decide with the resident reads: read paths (read_paths.hip), read support per junction (junctions.hip) and transits (transits.hip; a REPEATS or NESTED step of a
// simplify schedule runs them too and duplicates what they resolve, repeats.hip), each ONE call over the
// context's one placement scratch (placement.hip, c->res.placement) and the one window placer below.
// Host code; included by api.inc, whose context, fail(), MDBG_ENTER and HandOver it uses; what is current is asked of c->res (results.inc).

// ---- the refusals the stages share -------------------------------------------------------------------------
static int refuse_multi_gpu(mdbg_ctx* c, const char* what_is) {      // what_is: "unitigs are", "node sequences are", ...
    if (!(c->routed || c->own_world > 1)) return MDBG_OK;
    char buf[160]; snprintf(buf, sizeof buf, "%s single-GPU only: not available on a routed or partitioned context", what_is);
    return fail(c, MDBG_E_STATE, buf);
}
static int refuse_without_kept_reads(mdbg_ctx* c) {
    return c->P.flags & MDBG_FLAG_KEEP_READS ? MDBG_OK : fail(c, MDBG_E_STATE, "the context does not keep its reads (create it with MDBG_FLAG_KEEP_READS)");
}
static int refuse_without_unitig_list(mdbg_ctx* c) {
    return c->res.unitig_list_current() ? MDBG_OK : fail(c, MDBG_E_STATE, "no current unitig list on this context (call mdbg_graph_unitigs* or mdbg_graph_simplify* first)");
}
// device time of a stage's last call (of_stage: the `ms` of its result in c->res; read under the lock)
static int last_ms(mdbg_ctx* c, const double* of_stage, double* ms) {
    if (!c || !ms) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    *ms = *of_stage;
    return MDBG_OK;
}
// the five arrays of an edge list: the edge stage's own, and the unitig list's
static void hand_over_edges(HandOver& ho, const EdgeResult& r, EdgeColumns& h, mdbg_edge_list* out) {
    ho.col(r.n1, r.n, h.n1, &out->n1); ho.col(r.o1, r.n, h.o1, &out->o1); ho.col(r.n2, r.n, h.n2, &out->n2); ho.col(r.o2, r.n, h.o2, &out->o2); ho.col(r.overlap, r.n, h.ov, &out->overlap);
}

// ---- what the stages that decide with the resident reads share (read paths, junction support, transits, an EDGES step) ----
// roff[r] where the host knows it without asking the device: r is the first slot of a batch, or one past its last
static bool known_read_offset(const mdbg_ctx* c, u64 r, u64* v) {
    for (const Batch& b : c->batches) {
        if (b.slot0 == r) { *v = b.m0; return true; }
        if ((u64)b.slot0 + b.n_reads == r) { *v = b.m1; return true; }
    }
    return false;
}
// The window placer, the ONE way a stage reaches place_windows_kernel (main translation unit, beside the table): the range of reads with its minimizer indices and
// the store's arrays, as store_range fills them, and the launch placement_queue asks for.
struct PlaceWindows { mdbg_ctx* c; FinArgs F; ReadPathRange rg; };
static void place_windows(void* ctx, const ReadPathPlan& plan, hipStream_t s) {
    const PlaceWindows& p = *(const PlaceWindows*)ctx;
    launch_place_windows(table_args(p.c), p.F, p.c->fin_words, plan, p.F.mh, p.F.mread, p.F.roff, p.rg.i0, p.rg.i1, s);
}
// What a stage asks of the store before it places a window, for a list of n_unitigs unitigs and n_entries entries: the bounds, the range of reads with its minimizer
// indices, the store's arrays.  *empty <- the call answers MDBG_OK with zero counts (an empty context, an empty list, a range behind the store).  An EDGES step of a
// simplify schedule (unitigs_impl) asks it for the lists it is going to build, which have at most as many entries as the table has rows.
static int store_range(mdbg_ctx* c, uint64_t n_unitigs, uint64_t n_entries, uint64_t first_read, uint64_t max_reads, PlaceWindows* pw, bool* empty) {
    *empty = true;
    Results& R = c->res;
    if (!R.table_or_empty_context(nothing_resident(c))) return fail(c, MDBG_E_STATE, "the node table the unitig list was built from is not current");
    if (n_unitigs == 0 || first_read >= c->n_slots) return MDBG_OK;
    if (n_entries >= (1ull << 30) || R.n_rows() >= (1ull << 30)) return fail(c, MDBG_E_CAPACITY, "more than 2^30 nodes");
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
    pw->c = c; pw->F = F; pw->rg = rg; *empty = false;
    return MDBG_OK;
}
static int refuse_too_many_records(mdbg_ctx* c, uint64_t n_records) {
    return n_records < 0xFFFFFFF0ull ? MDBG_OK : fail(c, MDBG_E_CAPACITY, "more than 2^32 edge records");
}
// The prologue of a read-path, junction or transit call (what_is: "read paths are", ...): the device time of the stage's last call <- 0, the two refusals, the
// store's range for the current list and, for a stage with records, the bound on the list's edge records.
static int stage_prologue(mdbg_ctx* c, const char* what_is, uint64_t first_read, uint64_t max_reads, bool with_records, double* ms, PlaceWindows* pw, bool* empty) {
    *ms = 0; *empty = true;
    int e;
    if ((e = refuse_multi_gpu(c, what_is)) || (e = refuse_without_unitig_list(c))) return e;
    if (c->res.unitig_list_copies())
        return fail(c, MDBG_E_STATE, "the current unitig list holds copies made by a REPEATS or NESTED step: a row of the node table belongs to several entries, so no read can be placed on it");
    const UnitigResult& ul = c->res.unitigs.last;
    if ((e = store_range(c, ul.n_unitigs, ul.n_entries, first_read, max_reads, pw, empty)) || *empty) return e;
    return with_records ? refuse_too_many_records(c, ul.edges.n) : MDBG_OK;
}
// the defect mask of a stage (RP_DEFECT_* | JX_DEFECT_EDGE | TX_DEFECT_SHAPE) as the call's answer
static int stage_defect(mdbg_ctx* c, uint32_t defect) {
    if (defect & JX_DEFECT_EDGE) return fail(c, MDBG_E_DEVICE, "an edge record of the unitig list names a unitig outside the list");
    if (defect & TX_DEFECT_SHAPE) return fail(c, MDBG_E_DEVICE, "two explained crossings in a row do not walk all of one unitig: the edge records are not those of the unitig list");
    if (defect & RP_DEFECT_ENTRY) return fail(c, MDBG_E_DEVICE, "an entry of the unitig list names a node index that is not a row of the node table");
    if (defect & RP_DEFECT_PROBE) return fail(c, MDBG_E_DEVICE, "a probe sequence of the read paths visited every slot of the table");
    if (defect & RP_DEFECT_ROW) return fail(c, MDBG_E_DEVICE, "a solid slot's first sighting is no row of the node table");
    return MDBG_OK;
}

// ---- graph edges of the last finalized node table (edges.hip) -------------------------------------------
static int edges_impl(mdbg_ctx* c, float presimp, mdbg_edge_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    if (!(presimp >= 0.0f)) return fail(c, MDBG_E_PARAM, "presimp must be >= 0");
    memset(out, 0, sizeof *out);
    Results& R = c->res;
    if (!R.table_or_empty_context(nothing_resident(c))) return fail(c, MDBG_E_STATE, "no finalized node table on this context (call mdbg_finalize / mdbg_finalize_device first)");
    R.invalidate(FROM_EDGES); R.edge_list_is(EdgeResult{}, R.has_rows_table() && R.n_rows() == 0);      // until one is built: the empty list, current only for a table of no rows
    if (R.n_rows() == 0) return MDBG_OK;
    if (R.n_rows() >= (1ull << 30)) return fail(c, MDBG_E_CAPACITY, "more than 2^30 nodes");
    const FinArgs& F = c->finF;
    EdgeNodes nd; nd.keys = F.o_keys; nd.index = F.o_index; nd.abund = F.o_abund; nd.seqlen = F.o_seqlen; nd.shift = F.o_shift; nd.n = R.n_rows(); nd.k = c->P.k;
    EdgeResult r;
    HIPCHK(c, build_edges(R.edges.buf.get(), nd, presimp, c->stream, &r));
    R.edge_list_is(r, true);
    out->n = r.n; out->presimp_removed = r.presimp_removed;
    HandOver ho{c, "host copy of the edge list", to_host};
    hand_over_edges(ho, r, R.edges.h, out);
    return ho.err;
}
int mdbg_graph_edges(mdbg_ctx* c, float presimp, mdbg_edge_list* out) { return edges_impl(c, presimp, out, true); }
int mdbg_graph_edges_device(mdbg_ctx* c, float presimp, mdbg_edge_list* out) { return edges_impl(c, presimp, out, false); }

// ---- unitigs + base-space copy plan of the last node table and edge list (unitigs.hip) -------------------
// steps == nullptr: plain compaction (mdbg_graph_unitigs); otherwise the schedule runs first (mdbg_graph_simplify, simplify.hip) and stats is filled
static int unitigs_impl(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats, bool to_host) {
    MDBG_ENTER(c, out && !(stats && n_steps && !steps));
    memset(out, 0, sizeof *out);
    Results& R = c->res;
    auto& UL = R.unitigs;
    bool with_components = false, with_edges = false, with_repeats = false, with_nested = false;      // with_repeats: a REPEATS step was seen; with_nested: a NESTED step
    if (stats) {
        memset(stats, 0, sizeof *stats);
        for (uint32_t i = 0; i < n_steps; ++i) {
            const uint32_t kind = steps[i].kind;
            if (kind != MDBG_SIMPLIFY_TIPS && kind != MDBG_SIMPLIFY_BUBBLES && kind != MDBG_SIMPLIFY_COMPONENTS && kind != MDBG_SIMPLIFY_EDGES && kind != MDBG_SIMPLIFY_REPEATS && kind != MDBG_SIMPLIFY_SUPERBUBBLES && kind != MDBG_SIMPLIFY_NESTED)
                return fail(c, MDBG_E_PARAM, "unknown kind of simplification step");
            if (kind == MDBG_SIMPLIFY_REPEATS && (steps[i].max_nodes == 0 || steps[i].max_bases != 0))
                return fail(c, MDBG_E_PARAM, "a repeat step takes {REPEATS, min_support >= 1, 0}");
            if (kind == MDBG_SIMPLIFY_REPEATS && with_repeats) return fail(c, MDBG_E_PARAM, "a schedule holds at most one REPEATS step: reads cannot be placed on copied nodes");
            if (kind == MDBG_SIMPLIFY_EDGES && with_repeats) return fail(c, MDBG_E_PARAM, "an EDGES step cannot follow a REPEATS step: reads cannot be placed on copied nodes");
            if (kind == MDBG_SIMPLIFY_NESTED && (steps[i].max_nodes == 0 || steps[i].max_bases != 0))
                return fail(c, MDBG_E_PARAM, "a nested repeat step takes {NESTED, min_support >= 1, 0}");
            if (kind == MDBG_SIMPLIFY_EDGES && with_nested) return fail(c, MDBG_E_PARAM, "an EDGES step cannot follow a NESTED step: edge pruning on a graph that holds copies is not built");
            if (kind == MDBG_SIMPLIFY_REPEATS && with_nested) return fail(c, MDBG_E_PARAM, "a REPEATS step cannot follow a NESTED step: REPEATS means the graph holds no copies (use NESTED)");
            with_repeats |= kind == MDBG_SIMPLIFY_REPEATS; with_nested |= kind == MDBG_SIMPLIFY_NESTED;
            if (kind == MDBG_SIMPLIFY_EDGES && (steps[i].max_nodes == 0 || steps[i].max_bases != 0))
                return fail(c, MDBG_E_PARAM, "an edge step takes {EDGES, min_support >= 1, 0}");
            with_edges |= kind == MDBG_SIMPLIFY_EDGES;
            if (kind == MDBG_SIMPLIFY_COMPONENTS && steps[i].max_nodes == 0 && steps[i].max_bases == 0)
                return fail(c, MDBG_E_PARAM, "a component step without a limit would remove the whole graph");
            with_components |= kind == MDBG_SIMPLIFY_COMPONENTS;
        }
        UL.removed_unitigs.assign(n_steps, 0); UL.removed_nodes.assign(n_steps, 0); UL.removed_edges.assign(n_steps, 0);
        stats->n_steps = n_steps; stats->unitigs_removed = UL.removed_unitigs.data(); stats->nodes_removed = UL.removed_nodes.data();
    }
    R.invalidate(FROM_UNITIGS); UL.last = UnitigResult{};
    { const int e = refuse_multi_gpu(c, "unitigs are"); if (e) return e; }
    if (nothing_resident(c)) { R.unitig_list_is(UnitigResult{}); return MDBG_OK; }      // empty context: empty list, whatever the flags say (results.inc)
    if (!R.edge_list_current()) return fail(c, MDBG_E_STATE, "no current edge list on this context (call mdbg_finalize* and mdbg_graph_edges* first)");
    if (R.n_rows() == 0) { R.unitig_list_is(UnitigResult{}); return MDBG_OK; }
    if (with_components) R.comps.buf.get();
    SimplifySupport sup{}; PlaceWindows pw{};
    with_repeats |= with_nested;                     // from here on: a step that runs the transit stage
    if (with_edges || with_repeats) {                // what the junction support and the transits ask, before anything of the schedule is launched
        int e; bool empty;
        if ((e = refuse_too_many_records(c, R.edges.last.n)) || (e = store_range(c, 1, R.n_rows(), 0, 0, &pw, &empty))) return e;
        sup.pb = R.placement.buf.get(); sup.index = c->finF.o_index; sup.n_rows = R.n_rows(); sup.range = pw.rg; sup.has_reads = !empty;
        sup.placer = WindowPlacer{place_windows, &pw};
        if (with_edges) { sup.jb = R.junctions.buf.get(); R.junctions.ms = 0; }
        if (with_repeats) { sup.tb = R.transits.buf.get(); R.transits.ms = 0; }
    }
    const FinArgs& F = c->finF;
    UnitigNodes nd; nd.index = F.o_index; nd.abund = F.o_abund; nd.shift_full = F.o_shift_full; nd.src_read = F.o_src_read; nd.src_start = F.o_src_start; nd.src_end = F.o_src_end;
    nd.reversed = F.o_rev; nd.n = R.n_rows();
    UnitigResult r; int broken = 0;
    SimplifyInfo si{};
    const hipError_t he = stats ? simplify_unitigs(UL.buf.get(), R.comps.buf.have(), with_edges || with_repeats ? &sup : nullptr, nd, R.edges.last, steps, n_steps, c->stream, &r, UL.removed_unitigs.data(),
                                                   UL.removed_nodes.data(), UL.removed_edges.data(), &si, &broken)
                                : build_unitigs(UL.buf.get(), nd, R.edges.last, c->stream, &r, &broken);
    if (he != hipSuccess) return fail_hip(c, "build_unitigs", he);
    if (with_edges) R.junctions.ms = si.junction_ms;
    if (with_repeats) R.transits.ms = si.transit_ms;
    if (with_nested && getenv("MDBG_NESTED_STATS"))      // (diagnostic, no part of the interface: mdbg_simplify_stats has no room for these four counts)
        fprintf(stderr, "mdbg nested: ambiguous %llu resolved %llu conflicts %llu unanchored %llu\n", (unsigned long long)si.ambiguous, (unsigned long long)si.resolved,
                (unsigned long long)si.conflicts, (unsigned long long)si.unanchored);
    if (broken && si.junction_defect) return stage_defect(c, si.junction_defect);
    if (broken && si.transit_defect) return stage_defect(c, si.transit_defect);
    if (broken && si.repeats_too_large) return fail(c, MDBG_E_CAPACITY, "the copies of a REPEATS step or NESTED step would bring the graph to 2^30 nodes or 2^32 edge records");
    if (broken && si.repeats_defect)
        return fail(c, MDBG_E_DEVICE, si.repeats_defect & RX_DEFECT_MATCH ? "an end of an edge record at a resolved unitig belongs to no strong transit key, or to two: nothing was copied"
                                                                             : "a vertex of the last compaction or a transit row lies outside the unitig list: nothing was copied");
    if (broken) return fail(c, MDBG_E_DEVICE, "unitig ranking did not settle within ceil(log2(2n)) + 1 rounds, a union-find of a component step ran into its bound, a superbubble step met a vertex outside the list, or the walk broke an invariant");
    if (stats) {
        stats->n_compactions = si.n_compactions; stats->n_rounds_total = si.n_rounds_total; stats->n_syncs = si.n_syncs;
        for (uint32_t i = 0; i < n_steps; ++i) { stats->total_unitigs_removed += UL.removed_unitigs[i]; stats->total_nodes_removed += UL.removed_nodes[i]; }
    }
    R.unitig_list_is(r, si.copies);
    const u64 U = r.n_unitigs, N = r.n_entries;
    out->n_unitigs = U; out->n_entries = N; out->n_rounds = r.n_rounds; out->edges.n = r.edges.n;
    if (U == 0) return MDBG_OK;                      // a schedule that removed everything: the empty list, as an empty context gives it
    HandOver ho{c, "host copy of the unitig list", to_host};
    ho.col(r.offsets, U + 1, UL.off, &out->offsets);
    ho.col(r.node, N, UL.node, &out->node);
    ho.col(r.ori, N, UL.ori, &out->ori);
    ho.col(r.src_read, N, UL.sread, &out->src_read);
    ho.col(r.src_begin, N, UL.sbegin, &out->src_begin);
    ho.col(r.len, N, UL.len, &out->len);
    ho.col(r.revcomp, N, UL.rc, &out->revcomp);
    ho.col(r.dst_offset, N, UL.dst, &out->dst_offset);
    ho.col(r.length, U, UL.length, &out->length);
    ho.col(r.kc_sum, U, UL.kc, &out->kc_sum);
    ho.col(r.circular, U, UL.circ, &out->circular);
    hand_over_edges(ho, r.edges, UL.he, &out->edges);
    return ho.err;
}
int mdbg_graph_unitigs(mdbg_ctx* c, mdbg_unitig_list* out) { return unitigs_impl(c, nullptr, 0, out, nullptr, true); }
int mdbg_graph_unitigs_device(mdbg_ctx* c, mdbg_unitig_list* out) { return unitigs_impl(c, nullptr, 0, out, nullptr, false); }
int mdbg_graph_simplify(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats) {
    return stats ? unitigs_impl(c, steps, n_steps, out, stats, true) : MDBG_E_PARAM;
}
int mdbg_graph_simplify_device(mdbg_ctx* c, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats) {
    return stats ? unitigs_impl(c, steps, n_steps, out, stats, false) : MDBG_E_PARAM;
}
int mdbg_simplify_edges_removed(mdbg_ctx* c, const uint64_t** per_step, uint64_t* total) {
    if (!c) return MDBG_E_PARAM;
    MDBG_LOCK(c);
    const std::vector<u64>& v = c->res.unitigs.removed_edges;
    if (per_step) *per_step = v.data();
    if (total) { *total = 0; for (u64 x : v) *total += x; }
    return MDBG_OK;
}

// ---- connected components of the current unitig list (components.hip) -------------------------------------
static int components_impl(mdbg_ctx* c, mdbg_component_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    int e;
    if ((e = refuse_multi_gpu(c, "components are")) || (e = refuse_without_unitig_list(c))) return e;
    auto& K = c->res.comps;
    if (c->res.unitigs.last.n_unitigs == 0) return MDBG_OK;
    ComponentResult r; int broken = 0;
    const hipError_t he = build_components(K.buf.get(), c->res.unitigs.last, c->stream, &r, &broken);
    if (he != hipSuccess) return fail_hip(c, "build_components", he);
    if (broken) return fail(c, MDBG_E_DEVICE, "the union-find of the components ran into its bound of n_unitigs + 1 steps, or an edge names a unitig outside the list");
    const u64 U = r.n_unitigs, NC = r.n_components;
    out->n_unitigs = U; out->n_components = NC;
    HandOver ho{c, "host copy of the component list", to_host};
    ho.col(r.component, U, K.comp, &out->component);
    ho.col(r.first_unitig, NC, K.first, &out->first_unitig);
    ho.col(r.unitigs, NC, K.unitigs, &out->unitigs);
    ho.col(r.nodes, NC, K.nodes, &out->nodes);
    ho.col(r.bases, NC, K.bases, &out->bases);
    ho.col(r.kc_sum, NC, K.kc, &out->kc_sum);
    ho.col(r.circular, NC, K.circ, &out->circular);
    return ho.err;
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
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    int e;
    if ((e = refuse_without_kept_reads(c)) || (e = refuse_multi_gpu(c, "contigs are")) || (e = refuse_without_unitig_list(c))) return e;
    std::vector<KeptDesc> tab;
    if ((e = kept_table(c, tab))) return e;
    auto& C = c->res.contigs;
    ContigResult r;
    const hipError_t he = stitch_contigs(C.buf.get(), c->res.unitigs.last, tab.data(), (u32)tab.size(), min_len, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "stitch_contigs", he);
    C.ms = r.ms_stitch;
    if (r.err & 1u) return fail(c, MDBG_E_STATE, "an entry of the copy plan names a read that is not kept");
    if (r.err & 2u) return fail(c, MDBG_E_PARAM, "an entry of the copy plan lies outside its read (not the reads the table was built from)");
    out->n_contigs = r.n_contigs; out->n_bases = r.n_bases;
    HandOver ho{c, "host copy of the contigs", to_host};
    ho.col(r.bases, r.n_bases, C.bases, &out->bases);
    ho.col(r.offsets, r.n_contigs + 1, C.off, &out->offsets);      // (offsets: never empty)
    ho.col(r.unitig, r.n_contigs, C.unitig, &out->unitig);
    return ho.err;
}
int mdbg_graph_contigs(mdbg_ctx* c, uint64_t min_len, mdbg_contig_seqs* out) { return contigs_impl(c, min_len, out, true); }
int mdbg_graph_contigs_device(mdbg_ctx* c, uint64_t min_len, mdbg_contig_seqs* out) { return contigs_impl(c, min_len, out, false); }
int mdbg_contigs_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.contigs.ms : nullptr, ms); }

// ---- the node table's sequences gathered on the GPU from the resident read store, in bounded chunks (node_seqs.hip) ----
static int node_seqs_impl(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    out->first_row = first_row;
    int e;
    if ((e = refuse_without_kept_reads(c)) || (e = refuse_multi_gpu(c, "node sequences are"))) return e;
    Results& R = c->res;
    if (!R.table_finalized())
        return fail(c, MDBG_E_STATE, "no finalized node table on this context (call mdbg_finalize* first; an ingest, rewind or reset call ends the table)");
    std::vector<KeptDesc> tab;
    if ((e = kept_table(c, tab))) return e;
    auto& S = R.nseq;
    const FinArgs& F = c->finF;
    NodeSeqRows rows; rows.src_read = F.o_src_read; rows.src_start = F.o_src_start; rows.src_end = F.o_src_end; rows.reversed = F.o_rev; rows.n = R.n_rows();      // (none after the finalize of an empty context)
    hipError_t he;
    if (!R.prefix_summed() && rows.n) {              // once per node table
        he = node_seq_prefix(S.buf.get(), rows, c->stream);
        if (he != hipSuccess) return fail_hip(c, "node_seq_prefix", he);
        R.prefix_is_summed();
    }
    NodeSeqResult r;
    he = node_seq_chunk(S.buf.get(), rows, tab.data(), (u32)tab.size(), first_row, max_rows, max_bases, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "node_seq_chunk", he);
    S.ms = r.ms_gather;
    if (r.err & 1u) return fail(c, MDBG_E_STATE, "a row of the node table names a read that is not kept");
    if (r.err & 2u) return fail(c, MDBG_E_PARAM, "a row of the node table lies outside its read (not the reads the table was built from)");
    out->n_rows = r.n_rows; out->n_bases = r.n_bases;
    HandOver ho{c, "host copy of the node sequences", to_host};
    ho.col(r.bases, r.n_bases, S.bases, &out->bases);
    ho.col(r.offsets, r.n_rows + 1, S.off, &out->offsets);      // (offsets: never empty)
    return ho.err;
}
int mdbg_graph_node_seqs(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out) { return node_seqs_impl(c, first_row, max_rows, max_bases, out, true); }
int mdbg_graph_node_seqs_device(mdbg_ctx* c, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out) { return node_seqs_impl(c, first_row, max_rows, max_bases, out, false); }
int mdbg_node_seqs_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.nseq.ms : nullptr, ms); }

// ---- the resident reads threaded through the current unitig list (read_paths.hip) ---------
static int read_paths_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    out->first_read = first_read;
    Results& R = c->res;
    auto& P = R.rpaths;
    PlaceWindows pw; bool empty;
    const int e = stage_prologue(c, "read paths are", first_read, max_reads, false, &P.ms, &pw, &empty);
    if (e || empty) return e;
    ReadPathResult r;
    const hipError_t he = read_paths_run(P.buf.get(), R.placement.buf.get(), R.unitigs.last, pw.F.o_index, R.n_rows(), pw.rg, WindowPlacer{place_windows, &pw}, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "read_paths_run", he);
    P.ms = r.ms;
    if (r.defect) return stage_defect(c, r.defect);
    const u64 nr = r.n_reads, ns = r.n_steps, U = r.n_unitigs;
    out->n_reads = nr; out->n_windows = r.n_windows; out->n_placed = r.n_placed; out->n_steps = ns; out->n_unitigs = U;
    HandOver ho{c, "host copy of the read paths", to_host};
    ho.col(r.ordinal, nr, P.ord, &out->ordinal);
    ho.col(r.read_windows, nr, P.rw, &out->read_windows);
    ho.col(r.step_offsets, nr + 1, P.off, &out->step_offsets);
    ho.col(r.first_window, ns, P.fw, &out->first_window);
    ho.col(r.step_windows, ns, P.nw, &out->step_windows);
    ho.col(r.unitig, ns, P.unitig, &out->unitig);
    ho.col(r.first_entry, ns, P.fe, &out->first_entry);
    ho.col(r.strand, ns, P.strand, &out->strand);
    ho.col(r.support_windows, U, P.supw, &out->support_windows);
    ho.col(r.support_steps, U, P.sups, &out->support_steps);
    return ho.err;
}
int mdbg_graph_read_paths(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out) { return read_paths_impl(c, first_read, max_reads, out, true); }
int mdbg_graph_read_paths_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out) { return read_paths_impl(c, first_read, max_reads, out, false); }
int mdbg_read_paths_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.rpaths.ms : nullptr, ms); }

// ---- read support per junction of the current unitig list (junctions.hip) -----------------
static int junctions_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_junction_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    out->first_read = first_read;
    Results& R = c->res;
    auto& J = R.junctions;
    PlaceWindows pw; bool empty;
    const int e = stage_prologue(c, "junctions are", first_read, max_reads, true, &J.ms, &pw, &empty);
    if (e || empty) return e;
    JunctionResult r;
    const hipError_t he = junctions_run(J.buf.get(), R.placement.buf.get(), R.unitigs.last, pw.F.o_index, R.n_rows(), pw.rg, WindowPlacer{place_windows, &pw}, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "junctions_run", he);
    J.ms = r.ms;
    if (r.defect) return stage_defect(c, r.defect);
    const u64 nrec = r.n_records, nm = r.n_missing;
    out->n_reads = r.n_reads; out->n_adjacent = r.n_adjacent; out->n_links = r.n_links; out->n_crossings = r.n_crossings; out->n_explained = r.n_explained;
    out->n_missing_crossings = r.n_missing_crossings; out->n_records = nrec; out->n_missing = nm;
    HandOver ho{c, "host copy of the junction support", to_host};
    ho.col(r.support, nrec, J.support, &out->support);
    ho.col(r.missing_unitig1, nm, J.u1, &out->missing_unitig1);
    ho.col(r.missing_entry1, nm, J.e1, &out->missing_entry1);
    ho.col(r.missing_strand1, nm, J.s1, &out->missing_strand1);
    ho.col(r.missing_unitig2, nm, J.u2, &out->missing_unitig2);
    ho.col(r.missing_entry2, nm, J.e2, &out->missing_entry2);
    ho.col(r.missing_strand2, nm, J.s2, &out->missing_strand2);
    ho.col(r.missing_count, nm, J.count, &out->missing_count);
    return ho.err;
}
int mdbg_graph_junctions(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_junction_list* out) { return junctions_impl(c, first_read, max_reads, out, true); }
int mdbg_graph_junctions_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_junction_list* out) { return junctions_impl(c, first_read, max_reads, out, false); }
int mdbg_junctions_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.junctions.ms : nullptr, ms); }

// ---- reads that span a unitig end to end, and the repeats they resolve (transits.hip) ------
static int transits_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint64_t min_support, mdbg_transit_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    if (min_support == 0) return fail(c, MDBG_E_PARAM, "min_support must be >= 1");
    memset(out, 0, sizeof *out);
    out->first_read = first_read;
    Results& R = c->res;
    auto& T = R.transits;
    PlaceWindows pw; bool empty;
    const int e = stage_prologue(c, "transits are", first_read, max_reads, true, &T.ms, &pw, &empty);
    if (e || empty) return e;
    TransitResult r;
    const hipError_t he = transits_run(T.buf.get(), R.placement.buf.get(), R.unitigs.last, pw.F.o_index, R.n_rows(), pw.rg, min_support, WindowPlacer{place_windows, &pw}, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "transits_run", he);
    T.ms = r.ms;
    if (r.defect) return stage_defect(c, r.defect);
    const u64 nt = r.n_transits, U = r.n_unitigs;
    out->n_reads = r.n_reads; out->n_crossings = r.n_crossings; out->n_explained = r.n_explained; out->n_passes = r.n_passes; out->n_transits = nt;
    out->n_unitigs = U; out->n_repeats = r.n_repeats; out->n_resolved = r.n_resolved;
    HandOver ho{c, "host copy of the transits", to_host};
    ho.col(r.unitig, nt, T.unitig, &out->unitig);
    ho.col(r.in_unitig, nt, T.iu, &out->in_unitig);
    ho.col(r.in_entry, nt, T.ie, &out->in_entry);
    ho.col(r.in_strand, nt, T.is, &out->in_strand);
    ho.col(r.out_unitig, nt, T.ou, &out->out_unitig);
    ho.col(r.out_entry, nt, T.oe, &out->out_entry);
    ho.col(r.out_strand, nt, T.os, &out->out_strand);
    ho.col(r.in_record, nt, T.irec, &out->in_record);
    ho.col(r.out_record, nt, T.orec, &out->out_record);
    ho.col(r.count, nt, T.count, &out->count);
    ho.col(r.n_in, U, T.n_in, &out->n_in);
    ho.col(r.n_out, U, T.n_out, &out->n_out);
    ho.col(r.passes, U, T.passes, &out->passes);
    ho.col(r.verdict, U, T.verdict, &out->verdict);
    return ho.err;
}
int mdbg_graph_transits(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint64_t min_support, mdbg_transit_list* out) { return transits_impl(c, first_read, max_reads, min_support, out, true); }
int mdbg_graph_transits_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint64_t min_support, mdbg_transit_list* out) { return transits_impl(c, first_read, max_reads, min_support, out, false); }
int mdbg_transits_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.transits.ms : nullptr, ms); }

// ---- alignments: the steps chained over edge records, with base coordinates (alignments.hip; include/mdbg_align.h) ------
// The stage over the range of `pw`, and the hand-over of both results it fills: the read paths' (whose step columns the list shares) and its own.
// *dev_rp / *dev_al (optional) <- the two device results, for a stage that goes on from them on the device (the chains below).
static int alignments_over(mdbg_ctx* c, PlaceWindows& pw, mdbg_alignment_list* out, bool to_host, ReadPathResult* dev_rp = nullptr, AlignmentResult* dev_al = nullptr) {
    Results& R = c->res;
    auto& P = R.rpaths; auto& A = R.alns;
    const FinArgs& F = pw.F;
    AlignmentNodes nd; nd.index = F.o_index; nd.src_start = F.o_src_start; nd.src_end = F.o_src_end; nd.n_rows = R.n_rows(); nd.positions = c->mpos.as<u32>(); nd.l = c->P.l;
    ReadPathResult rp; AlignmentResult r;
    const hipError_t he = alignments_run(A.buf.get(), P.buf.get(), R.placement.buf.get(), R.unitigs.last, nd, pw.rg, WindowPlacer{place_windows, &pw}, c->stream, &rp, &r);
    if (he != hipSuccess) return fail_hip(c, "alignments_run", he);
    A.ms = P.ms = r.ms;
    if (r.defect & AL_DEFECT_RECORD) return fail(c, MDBG_E_DEVICE, "a record an alignment needs is absent or outside the list (the closing record of a ring a step wraps), or a window reaches past its range");
    if (r.defect) return stage_defect(c, r.defect);
    if (dev_rp) *dev_rp = rp;
    if (dev_al) *dev_al = r;
    const u64 nr = rp.n_reads, ns = rp.n_steps, na = r.n_alignments;
    out->n_reads = nr; out->n_windows = rp.n_windows; out->n_placed = rp.n_placed; out->n_steps = ns; out->n_chained = r.n_chained; out->n_alignments = na; out->n_wraps = r.n_wraps;
    out->n_unitigs = rp.n_unitigs;
    HandOver ho{c, "host copy of the alignments", to_host};
    ho.col(rp.ordinal, nr, P.ord, &out->ordinal);
    ho.col(rp.read_windows, nr, P.rw, &out->read_windows);
    ho.col(rp.step_offsets, nr + 1, P.off, &out->step_offsets);
    ho.col(rp.first_window, ns, P.fw, &out->first_window);
    ho.col(rp.step_windows, ns, P.nw, &out->step_windows);
    ho.col(rp.unitig, ns, P.unitig, &out->unitig);
    ho.col(rp.first_entry, ns, P.fe, &out->first_entry);
    ho.col(rp.strand, ns, P.strand, &out->strand);
    ho.col(r.step_record, ns, A.srec, &out->step_record);
    ho.col(r.aln_offsets, nr + 1, A.aoff, &out->aln_offsets);
    ho.col(r.aln_step_offsets, na + 1, A.asoff, &out->aln_step_offsets);
    ho.col(r.aln_windows, na, A.awin, &out->aln_windows);
    ho.col(r.query_begin, na, A.qbeg, &out->query_begin);
    ho.col(r.query_end, na, A.qend, &out->query_end);
    ho.col(r.path_length, na, A.plen, &out->path_length);
    ho.col(r.path_begin, na, A.pbeg, &out->path_begin);
    ho.col(r.path_end, na, A.pend, &out->path_end);
    return ho.err;
}
static int alignments_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_alignment_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    out->first_read = first_read;
    PlaceWindows pw; bool empty;
    c->res.rpaths.ms = 0;
    const int e = stage_prologue(c, "alignments are", first_read, max_reads, true, &c->res.alns.ms, &pw, &empty);
    if (e || empty) return e;
    return alignments_over(c, pw, out, to_host);
}
int mdbg_graph_alignments(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_alignment_list* out) { return alignments_impl(c, first_read, max_reads, out, true); }
int mdbg_graph_alignments_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, mdbg_alignment_list* out) { return alignments_impl(c, first_read, max_reads, out, false); }
int mdbg_alignments_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.alns.ms : nullptr, ms); }

// a batch that is not resident: sketched behind the store as mdbg_query_batch does it, aligned, and the store rolled back (StoreRollback, store.inc)
// chain != null: the chain stage behind it (mdbg_graph_chain_batch); out is then chain->out's alignment list
struct ChainCall { uint32_t max_skew, max_gap; mdbg_chain_list* out; };
static int chains_behind(mdbg_ctx* c, PlaceWindows& pw, const ChainCall& cc, bool to_host);
static int align_batch_impl(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, mdbg_alignment_list* out, bool to_host, const ChainCall* chain = nullptr) {
    if (!c || !out) return MDBG_E_PARAM;
    u64 nb = 0;
    StageHold hold;
    if (n_reads) { int e = stage_host_batch(c, bases, offsets, n_reads, &nb, hold); if (e) return e; }
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (chain) { memset(chain->out, 0, sizeof *chain->out); c->res.chains.ms = 0; } else memset(out, 0, sizeof *out);
    Results& R = c->res;
    R.rpaths.ms = 0; R.alns.ms = 0;
    int e;
    if ((e = refuse_multi_gpu(c, chain ? "chains are" : "alignments are")) || (e = refuse_without_unitig_list(c))) return e;
    if (R.unitig_list_copies()) return fail(c, MDBG_E_STATE, "the current unitig list holds copies made by a REPEATS or NESTED step: no read can be placed on it");
    if (!R.table_or_empty_context(nothing_resident(c))) return fail(c, MDBG_E_STATE, "the node table the unitig list was built from is not current");
    if (n_reads == 0) return MDBG_OK;
    const auto held = R.held();                      // the sketch ends the unitig list (an ingest); the rollback below makes the store what the list was built on again
    struct Restore { Results& R; decltype(held) h; ~Restore() { R.still_holds(h); } } restore{R, held};
    // sketch into the resident store behind everything that is there, align exactly that batch; the store is rolled back on every way out of this block
    const StoreRollback tmp(c);
    e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, 0);
    if (e) { if (e == MDBG_E_ALPHABET) c->poisoned = 0; return e; }          // a bad byte in a query does not poison the node table; a device error does
    R.still_holds(held);                             // (the stage below asks whether the list is current)
    const Batch b = c->batches.back();
    const UnitigResult& ul = R.unitigs.last;
    PlaceWindows pw; bool empty;
    if ((e = store_range(c, ul.n_unitigs, ul.n_entries, b.slot0, 0, &pw, &empty)) || empty) return e;
    if ((e = refuse_too_many_records(c, ul.edges.n))) return e;
    pw.rg.by_slot0 = nullptr; pw.rg.by_slot_first = nullptr; pw.rg.n_batches = 0;      // the temporary batch is in no batch table: ordinal[q] = q (reads_kernel)
    return chain ? chains_behind(c, pw, *chain, to_host) : alignments_over(c, pw, out, to_host);
}
int mdbg_graph_align_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, mdbg_alignment_list* out) { return align_batch_impl(c, bases, offsets, n_reads, out, true); }
int mdbg_graph_align_batch_device(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, mdbg_alignment_list* out) { return align_batch_impl(c, bases, offsets, n_reads, out, false); }

// ---- chains: consecutive alignments of a read joined over a bridge (chains.hip; include/mdbg_chain.h) ------
// The alignment stage over the range of `pw`, the chain stage behind it on what that left on the device, and the hand-over of the three results.
static int chains_behind(mdbg_ctx* c, PlaceWindows& pw, const ChainCall& cc, bool to_host) {
    Results& R = c->res;
    auto& K = R.chains;
    mdbg_chain_list* out = cc.out;
    ReadPathResult rp; AlignmentResult al;
    const int e = alignments_over(c, pw, &out->alignments, to_host, &rp, &al);
    if (e) return e;
    ChainResult r;
    const hipError_t he = chains_run(K.buf.get(), R.placement.buf.get(), R.unitigs.last, rp, al, c->P.l, cc.max_skew, cc.max_gap, c->stream, &r);
    if (he != hipSuccess) return fail_hip(c, "chains_run", he);
    K.ms = R.alns.ms + r.ms;
    if (r.defect) return fail(c, MDBG_E_DEVICE, "an alignment names a step, a unitig or a record outside its list");
    const u64 nr = rp.n_reads, na = al.n_alignments, nc = r.n_chains;
    out->n_bridges_inside = r.n_bridges_inside; out->n_bridges_record = r.n_bridges_record; out->n_bridges = r.n_bridges_inside + r.n_bridges_record;
    out->n_chains = nc; out->n_gap_windows = r.n_gap_windows;
    HandOver ho{c, "host copy of the chains", to_host};
    ho.col(r.bridge_record, na, K.brec, &out->bridge_record);
    ho.col(r.bridge_entries, na, K.bent, &out->bridge_entries);
    ho.col(r.chain_offsets, nr + 1, K.coff, &out->chain_offsets);
    ho.col(r.chain_aln_offsets, nc + 1, K.caoff, &out->chain_aln_offsets);
    ho.col(r.chain_windows, nc, K.cwin, &out->chain_windows);
    ho.col(r.chain_gap_windows, nc, K.cgap, &out->chain_gap_windows);
    ho.col(r.query_begin, nc, K.qbeg, &out->query_begin);
    ho.col(r.query_end, nc, K.qend, &out->query_end);
    ho.col(r.path_length, nc, K.plen, &out->path_length);
    ho.col(r.path_begin, nc, K.pbeg, &out->path_begin);
    ho.col(r.path_end, nc, K.pend, &out->path_end);
    return ho.err;
}
static int chains_impl(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out, bool to_host) {
    MDBG_ENTER(c, out);
    memset(out, 0, sizeof *out);
    out->alignments.first_read = first_read;
    PlaceWindows pw; bool empty;
    c->res.rpaths.ms = 0; c->res.chains.ms = 0;
    const int e = stage_prologue(c, "chains are", first_read, max_reads, true, &c->res.alns.ms, &pw, &empty);
    if (e || empty) return e;
    return chains_behind(c, pw, ChainCall{max_skew, max_gap, out}, to_host);
}
int mdbg_graph_chains(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out) { return chains_impl(c, first_read, max_reads, max_skew, max_gap, out, true); }
int mdbg_graph_chains_device(mdbg_ctx* c, uint64_t first_read, uint64_t max_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out) { return chains_impl(c, first_read, max_reads, max_skew, max_gap, out, false); }
int mdbg_chains_ms(mdbg_ctx* c, double* ms) { return last_ms(c, c ? &c->res.chains.ms : nullptr, ms); }
int mdbg_graph_chain_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out) {
    const ChainCall cc{max_skew, max_gap, out};
    return out ? align_batch_impl(c, bases, offsets, n_reads, &out->alignments, true, &cc) : MDBG_E_PARAM;
}
int mdbg_graph_chain_batch_device(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out) {
    const ChainCall cc{max_skew, max_gap, out};
    return out ? align_batch_impl(c, bases, offsets, n_reads, &out->alignments, false, &cc) : MDBG_E_PARAM;
}
