// ingest_api.inc — the sketch stage, the insertion round and the entry points over them: ingest / sketch / pack / query, reset / mark / rewind, l-mer filter, stats
namespace {
constexpr u64 SLAB_BUDGET = 6ull << 30;       // bytes of per-tile slabs per sketch launch (denser settings run in several launches)
int insert_resident_impl(mdbg_ctx* c, bool allow_pending = false);

// The closing decode of an insertion round, from the scalars the host read behind its launches: the fused tail of the sketch stage, the sliced round and the plain
// round end here.  probe_msg: what a probe error is reported as; ms: the round's insertion time, added once that first check has passed.
constexpr const char* TABLE_FULL = "the table filled up during insertion";
int close_round(mdbg_ctx* c, const u64* sc, const char* probe_msg, float ms) {
    if ((u32)sc[SC_PROBEERR]) return fail(c, MDBG_E_PARAM, probe_msg);
    c->ms_insert += ms;
    c->n_windows += sc[SC_BATCHWIN];
    c->n_distinct = sc[SC_NDISTINCT];
    // offsets of imported regions are validated on the device (mdbg_sketch_commit; clamped, so the kernels above stayed in bounds)
    if (sc[SC_IMPORTERR]) return fail(c, MDBG_E_PARAM, "read offsets of an imported sketch are not consistent with its size");
    if ((u32)sc[SC_CAPERR]) return fail(c, MDBG_E_CAPACITY, "a read has more than 2^26 minimizers");
    return MDBG_OK;
}

// ---- the sketch stage: its steps, then sketch_device_impl, the retry loop over them ----------------------------------------------------------------------
struct SketchCall {            // what the steps of one call share
    const SketchInput& in; const u64* d_offsets; u64 n_reads, n_bases, first_ordinal, n_tiles_total; u32 slot0; bool phase_dbg;
};
int check_sketch_call(mdbg_ctx* c, const SketchInput& in, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 first_ordinal, u64 n_tiles_total) {
    if (in.fmt == FMT_ASCII && !in.d_bases && n_bases) return fail(c, MDBG_E_PARAM, "null bases");
    if (in.fmt == FMT_PLANES && !in.d_planes && n_bases) return fail(c, MDBG_E_PARAM, "null packed words");
    if (!d_offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if ((((uintptr_t)in.d_bases) | ((uintptr_t)in.d_planes)) & 15) return fail(c, MDBG_E_PARAM, "device bases pointer must be 16-byte aligned");
    if (in.n_exc && (!in.d_exc_pos || !in.d_exc_val)) return fail(c, MDBG_E_PARAM, "null exception list");
    if (in.n_exc >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many exceptions");
    if (n_reads >= 0xFFFFFFF0ull || (u64)c->n_slots + n_reads >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "too many reads");
    if (first_ordinal + n_reads >= (1ull << (64 - WIN_BITS))) return fail(c, MDBG_E_CAPACITY, "read ordinal too large");
    if (n_tiles_total >= 0x7FFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "batch too large for one call");
    return MDBG_OK;
}
double density2(const mdbg_params& P) { double d = 2.0 * P.density; if (d > 1.0) d = 1.0; if (d < 0) d = 0; return d; }
// records per tile slab: expectation for i.i.d. hashes + 25 % + 6 sigma; a tile that still overflows makes the batch run again
// with slabs sized from the largest count seen (and the context remembers that size: slab_cap_min).  cap0_hook: MDBG_SLAB_CAP0, see sketch_device_impl
struct SlabPlan { u32 slab_cap, gather_tiles; };
SlabPlan slab_sizing(const mdbg_params& P, u32 slab_cap_min, u32 cap0_hook) {
    const u64 tile_bases = TILE_STRIDE;
    SlabPlan sp{0, 1};
    // syncmers: about one l-mer in l-s+1 has its smallest s-mer in the middle, of which a fraction `density` survives
    const double per_base = P.scheme == MDBG_SCHEME_SYNCMERS ? std::min(1.0, std::max(0.0, P.density)) / (P.syncmer_s ? std::max(1.0, (double)(P.l - P.syncmer_s + 1) / 2.0) : 1.0) : density2(P);
    const double e = (double)tile_bases * per_base; double v = e * 1.25 + 6.0 * sqrt(e) + 32.0; if (v > (double)tile_bases) v = (double)tile_bases; sp.slab_cap = ((u32)v + 7u) & ~7u;
    // small tiles: one gather wave takes several (about 256 expected records)
    if (e < 128.0) sp.gather_tiles = (u32)std::max(1.0, std::min(16.0, 256.0 / std::max(e, 1.0)));
    if (sp.slab_cap < slab_cap_min) sp.slab_cap = slab_cap_min;
    if (cap0_hook && !slab_cap_min) sp.slab_cap = std::max<u32>(8u, cap0_hook & ~7u);
    if (sp.slab_cap > (u32)tile_bases) sp.slab_cap = (u32)tile_bases;
    return sp;
}
// tiles per launch: the slabs of one launch stay under `budget` bytes (SLAB_BUDGET: one launch for every BASELINE configuration; dense settings
// run in several, one after the other).  Measured and dropped this round: cutting a batch into 2-4 parts whose scan + gather run on
// a second stream under the next part's tile kernel — the copy slows the tile kernel down by as much as it hides (profiles/r03_notes.md).
struct TileParts { u64 chunk = 1, max_part = 0; std::vector<u64> part_end; };      // part_end: exclusive end tile of every launch
TileParts partition_tiles(u64 n_tiles_total, u32 slab_cap, u64 budget) {
    TileParts tp;
    tp.chunk = std::max<u64>(1, std::min<u64>(n_tiles_total ? n_tiles_total : 1, budget / ((u64)slab_cap * sizeof(Rec))));
    for (u64 t0 = 0; t0 < n_tiles_total; t0 += tp.chunk) tp.part_end.push_back(std::min<u64>(n_tiles_total, t0 + tp.chunk));
    u64 t0 = 0; for (u64 e : tp.part_end) { tp.max_part = std::max(tp.max_part, e - t0); t0 = e; }
    return tp;
}
// per-tile state of a batch's tiles (the slabs, sized per attempt, are not part of it)
int ensure_tile_state(mdbg_ctx* c, u64 n_tiles_total, bool exceptions) {
    hipStream_t s = c->stream;
    HIPCHK(c, c->bread.ensure((n_tiles_total + 2) * 4, 0, s));
    HIPCHK(c, c->tile_recs.ensure(n_tiles_total * sizeof(TileRec), 0, s));
    HIPCHK(c, c->n_valid.ensure(n_tiles_total * 4, 0, s));
    HIPCHK(c, c->n_scan.ensure(n_tiles_total * 4, 0, s));
    HIPCHK(c, c->last_read.ensure(n_tiles_total * 4, 0, s));
    if (exceptions) HIPCHK(c, c->tile_flags.ensure(n_tiles_total, 0, s));
    return MDBG_OK;
}
// the gather of n slabs (slab_cap records each, n_valid[] of them filled) into the batch's place in the store; the tile launches add their scan inputs
GatherArgs gather_args(mdbg_ctx* c, const SketchCall& k, u32 tile0, u32 n, const Rec* slab, u32 slab_cap, const u32* n_valid, bool last_launch, u32 tiles_per_wave) {
    GatherArgs G{};
    G.tile0 = tile0; G.n = n; G.slab = slab; G.slab_cap = slab_cap; G.n_valid = n_valid;
    G.out_hash = c->mh.as<u64>(); G.out_pos = c->mpos.as<u32>(); G.out_read = c->mread.as<u32>(); G.out_cap = c->mcap;
    G.m0 = c->M; G.slot0 = k.slot0; G.n_reads = (u32)k.n_reads; G.off = c->roff.as<u64>(); G.last_launch = last_launch ? 1u : 0u;
    G.tiles_per_wave = tiles_per_wave;
    return G;
}
// MDBG_PHASE_TIMING: the tile kernel's per-phase cycle stamps, averaged over the tiles of the fast path
void dump_phase_timing(const SketchArgs& A, u32 slab_cap, hipStream_t s) {
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
// The tile and gather launches of one attempt (n_tiles_total > 0): fills in the tile side of A, prepares the tile records (which also sets the scalars of init0),
// then one tile launch and one gather per part
int launch_tiles(mdbg_ctx* c, const SketchCall& k, SketchArgs& A, SketchInit init0, const TileParts& tp, const SlabPlan& sp) {
    hipStream_t s = c->stream;
    const SketchInput& in = k.in;
    A.bread = c->bread.as<u32>(); A.recs = c->tile_recs.as<TileRec>(); A.n_tiles = (u32)k.n_tiles_total;
    A.slab = c->slab.as<Rec>(); A.slab_cap = sp.slab_cap; A.n_valid = c->n_valid.as<u32>(); A.n_scan = c->n_scan.as<u32>(); A.last_read = c->last_read.as<u32>(); A.over_max = (u32*)(scal(c) + SC_OVERMAX);
    A.t4 = c->d_t4.as<u64>();
    A.tile_flags = in.n_exc ? c->tile_flags.as<u8>() : nullptr;
    A.err_flag = (u32*)(scal(c) + SC_ERRFLAG); A.slow_total = (unsigned long long*)(scal(c) + SC_SLOWTOTAL);
    A.read_base = k.slot0; A.bound = c->bound; A.btop = (u32)(c->bound >> (64 - BS_B)); A.force_slow = ((c->P.flags & 1u) || c->P.l > (u32)BS_MAX_L) ? 1u : 0u;      // l > 32: the generic exact walker handles any l
    A.dbg = nullptr;
    { const char* sp_ = getenv("MDBG_STOP_PHASE"); A.stop_phase = sp_ ? (u32)atoi(sp_) : 0u; }
    if (k.phase_dbg) { HIPCHK(c, c->phase_dbg.ensure((size_t)k.n_tiles_total * 128, 0, s)); HIPCHK(c, hipMemsetAsync(c->phase_dbg.p, 0, (size_t)k.n_tiles_total * 128, s)); A.dbg = c->phase_dbg.as<u64>(); }
    // the first level of the gather's scan is accumulated by the tiles themselves (SketchArgs::block_sum; zeroed by the kernel that prepares the tile records)
    const u32 n_gran = (u32)((tp.max_part + SCAN_GRAN - 1) / SCAN_GRAN);
    HIPCHK(c, c->gran_sum.ensure((size_t)n_gran * 8 + 64, 0, s));
    A.block_sum = (unsigned long long*)c->gran_sum.as<u64>();
    init0.zero_arr = c->gran_sum.as<u64>(); init0.zero_arr_n = n_gran;
    launch_bread(k.d_offsets, (u32)k.n_reads, k.n_bases, A.n_tiles, c->bread.as<u32>(), c->tile_recs.as<TileRec>(), init0, s);
    if (in.n_exc) {
        HIPCHK(c, hipMemsetAsync(c->tile_flags.p, 0, k.n_tiles_total, s));
        launch_tile_flags(in.d_exc_pos, (u32)in.n_exc, A.n_tiles, c->tile_flags.as<u8>(), s);
    }
    if (c->P.scheme == MDBG_SCHEME_SYNCMERS) {
        A.scheme = 1; A.s = c->P.syncmer_s; A.btop = 0;
        const double v = c->P.density * (double)(1ull << (2 * c->P.l));           // src/read.rs:218, saturating cast
        A.bound = !(v > 0.0) ? 0 : (v >= 18446744073709551616.0 ? ~0ull : (u64)v);
        A.force_slow = ((c->P.flags & 1u) || c->P.syncmer_s > 13) ? 1u : 0u;      // the register window packs hash << 5 | age: s <= 13; longer s-mers take the generic machine
    }
    u64 t0 = 0;
    for (size_t pi = 0; pi < tp.part_end.size(); ++pi) {
        const u32 nt = (u32)(tp.part_end[pi] - t0);
        Rec* const part_slab = c->slab.as<Rec>();
        A.tile0 = (u32)t0; A.slab = part_slab;
        if (pi) HIPCHK(c, hipMemsetAsync(c->gran_sum.p, 0, (size_t)n_gran * 8, s));      // (several launches per batch — dense settings —: the next launch's sums start from zero)
        { hipEvent_t tb = next_tile_event(c), te = next_tile_event(c); launch_sketch(A, nt, s, tb, te); }
        GatherArgs G = gather_args(c, k, (u32)t0, nt, part_slab, sp.slab_cap, A.n_valid, pi + 1 == tp.part_end.size(), sp.gather_tiles);
        G.n_scan = A.n_scan; G.last_read = A.last_read;
        launch_gather(G, c->scan_tmp.as<u64>(), c->tile_base.as<u64>(), scal(c) + SC_CARRY, s, c->gran_sum.as<u64>());
        c->n_tile_launches += 1;
        t0 = tp.part_end[pi];
    }
    c->n_tile_bases += k.n_bases;
    if (k.phase_dbg) dump_phase_timing(A, sp.slab_cap, s);
    return MDBG_OK;
}
// a byte outside ACGTN was seen somewhere: apply the reference's exact rule (alphabet_rule_kernel)
int alphabet_rule_pass(mdbg_ctx* c, const SketchArgs& A, u64 first_ordinal) {
    hipStream_t s = c->stream;
    u64 which = ~0ull;
    HIPCHK(c, hipMemcpyAsync(scal(c) + SC_SLOWTOTAL, &which, 8, hipMemcpyHostToDevice, s));      // scratch use of a scalar that was read already
    launch_alphabet_rule(A, (unsigned long long*)(scal(c) + SC_SLOWTOTAL), s);
    HIPCHK(c, hipMemcpyAsync(&which, scal(c) + SC_SLOWTOTAL, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (which != ~0ull) {
        char buf[160]; snprintf(buf, sizeof buf, "Non-ACGTN nucleotide in read %llu of the batch (ordinal %llu)", (unsigned long long)which, (unsigned long long)(first_ordinal + which));
        return fail(c, MDBG_E_ALPHABET, buf);
    }
    return MDBG_OK;
}
// --lmer-counts: of the minimizers that passed the threshold keep those whose l-mer is in the set (read.rs:200-205); the
// survivors go through slabs of 256 and the sketch's gather back to the same place in the store.  m_new: end of the batch in the store, before and after
int lmer_filter_pass(mdbg_ctx* c, const SketchCall& k, u64& m_new) {
    hipStream_t s = c->stream;
    const SketchInput& in = k.in;
    const u64 init[1] = {c->M};
    const u32 nb = lmer_filter_blocks(m_new - c->M);
    HIPCHK(c, c->slab.ensure((size_t)nb * 256 * sizeof(Rec), 0, s));
    HIPCHK(c, c->n_valid.ensure((size_t)nb * 4, 0, s)); HIPCHK(c, c->tile_base.ensure((size_t)nb * 8, 0, s)); HIPCHK(c, c->scan_tmp.ensure(((size_t)nb / 1024 + 2) * 8, 0, s));
    LmerFilterArgs L{};
    L.set = c->lmer_set.as<u64>(); L.set_mask = c->lmer_mask; L.has_all_ones = c->lmer_all_ones;
    L.mh = c->mh.as<u64>(); L.mpos = c->mpos.as<u32>(); L.mread = c->mread.as<u32>(); L.m0 = c->M; L.m1 = m_new;
    L.offsets = k.d_offsets; L.slot0 = k.slot0; L.l = c->P.l; L.hpc = c->P.reads_already_hpc == 0 ? 1u : 0u;
    L.slab = c->slab.as<Rec>(); L.n_valid = c->n_valid.as<u32>();
    launch_lmer_filter(L, in.fmt, in.d_bases, in.d_planes, in.d_exc_pos, in.d_exc_val, (u32)in.n_exc, s);
    HIPCHK(c, hipMemcpyAsync(scal(c) + SC_CARRY, init, 8, hipMemcpyHostToDevice, s));
    const GatherArgs G = gather_args(c, k, 0, nb, L.slab, 256, L.n_valid, true, 1);      // the offsets of the filtered set replace the first pass's
    launch_gather(G, c->scan_tmp.as<u64>(), c->tile_base.as<u64>(), scal(c) + SC_CARRY, s);
    u64 sc[SC_N];
    int e = read_scalars(c, sc); if (e) return e;
    m_new = sc[SC_CARRY];
    return MDBG_OK;
}
// The insertion launched behind the batch's own sketch, before the host has looked at it: the window count and the capacity check in ONE launch
// (count_reserve_kernel), then the windows of whatever the sketch left between M and the device's SC_CARRY
int launch_fused_insert(mdbg_ctx* c, const SketchCall& k) {
    hipStream_t s = c->stream;
    u32* const ins_flags = (u32*)(scal(c) + SC_CAPERR);                // [0] window index overflow, [1] table too small / sketch to be repeated
    launch_count_reserve(c->roff.as<u64>(), k.slot0, (u32)k.n_reads, c->P.k, scal(c) + SC_BATCHWIN, (u32*)(scal(c) + SC_DONE), c->shards.as<u64>() + SH_DISTINCT * CTR_SHARDS, scal(c) + SC_NDISTINCT,
                         c->cap, ins_flags + 1, scal(c) + SC_CARRY, c->mcap, (const u32*)(scal(c) + SC_OVERMAX), s);
    if (!c->ev3) HIPCHK(c, hipEventCreate(&c->ev3));
    launch_insert_windows(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), c->M, c->mcap, k.slot0, k.first_ordinal, scal(c) + SC_NWINDOWS, ins_flags, s, scal(c) + SC_CARRY);
    STAGE_EVENT(c, c->ev3, s);
    return MDBG_OK;
}
// The table side of a round trip whose insertion rode behind the sketch (the tail of insert_resident_impl)
int fused_tail(mdbg_ctx* c, const u64* sc, bool* inserted) {
    c->res.invalidate(FROM_NODES);
    if (sc[SC_CAPERR] >> 32) return MDBG_OK;   // the sketch was fine, so the table was too small: nothing was inserted; the caller inserts the plain way (*inserted stays false)
    c->batches_inserted = c->batches.size();
    *inserted = true;
    float ms = 0;
    if (c->timing >= 2 && hipEventElapsedTime(&ms, c->ev1, c->ev3) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
    return close_round(c, sc, TABLE_FULL, ms);
}

// the sketch stage over a device-resident batch; appends to the resident store and records a Batch (store_append)
// then_insert: the caller inserts the batch's windows right away.  When nothing stands in the way (a table exists, one launch, no filter, nothing
// else pending) the window count, the capacity check and the insertion are launched BEHIND the sketch before the host has looked at it — one host
// round trip per batch instead of two; the device-side check also stops the insertion when the sketch has to be repeated.  *inserted tells the caller.
int sketch_device_impl(mdbg_ctx* c, const SketchInput& in, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 first_ordinal, bool then_insert = false, bool* inserted = nullptr) {
    if (inserted) *inserted = false;
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (n_reads == 0) return MDBG_OK;
    const u64 tile_bases = TILE_STRIDE;
    const u64 n_tiles_total = (n_bases + tile_bases - 1) / tile_bases;
    { int e = check_sketch_call(c, in, d_offsets, n_reads, n_bases, first_ordinal, n_tiles_total); if (e) return e; }
    hipStream_t s = c->stream;
    u32 slot0 = 0;
    { int e = next_slot0(c, c->M, n_reads, &slot0); if (e) return e; }
    // test hooks: MDBG_SLAB_CAP0 = slab size of a context's FIRST attempt (small: the tiles overflow and the batch runs again with slabs sized from what was seen),
    // MDBG_SLAB_BUDGET_MB = bytes of slabs per launch (small: several launches per batch)
    static const u32 cap0_hook = getenv("MDBG_SLAB_CAP0") ? (u32)atoi(getenv("MDBG_SLAB_CAP0")) : 0u;
    static const u64 budget_hook = getenv("MDBG_SLAB_BUDGET_MB") ? (u64)atoll(getenv("MDBG_SLAB_BUDGET_MB")) << 20 : 0ull;
    SlabPlan sp = slab_sizing(c->P, c->slab_cap_min, cap0_hook);
    if (n_tiles_total) { int e = ensure_tile_state(c, n_tiles_total, in.n_exc != 0); if (e) return e; }
    u64 want = c->M + (u64)((double)n_bases * density2(c->P) * 1.15) + 65536;
    const bool phase_dbg = getenv("MDBG_PHASE_TIMING") != nullptr;      // per-phase cycle stamps of the tile kernel (diagnostic)
    const SketchCall k{in, d_offsets, n_reads, n_bases, first_ordinal, n_tiles_total, slot0, phase_dbg};
    for (int attempt = 0; attempt < 4; ++attempt) {
        { int e = store_ensure(c, want); if (e) return e; }
        const TileParts tp = partition_tiles(n_tiles_total, sp.slab_cap, budget_hook ? budget_hook : SLAB_BUDGET);
        if (n_tiles_total) {
            HIPCHK(c, c->slab.ensure((size_t)tp.chunk * sp.slab_cap * sizeof(Rec), 0, s));
            HIPCHK(c, c->tile_base.ensure((size_t)tp.max_part * 8, 0, s));
            HIPCHK(c, c->scan_tmp.ensure(((size_t)tp.max_part / 1024 + 2) * 8, 0, s));
        }
        STAGE_EVENT(c, c->ev0, s);
        // SC_CARRY = M, the error / slow-tile / overflow scalars = 0: by the kernel that prepares the tile records (or a launch of their own)
        SketchInit init0{};
        init0.zero[0] = scal(c) + SC_ERRFLAG; init0.zero[1] = scal(c) + SC_SLOWTOTAL; init0.zero[2] = scal(c) + SC_OVERMAX; init0.set_p = scal(c) + SC_CARRY; init0.set_v = c->M;
        // the insertion can ride behind this sketch when its grid can be sized without the count: the store's free room is the bound, and it must not be
        // much more than the batch is expected to fill (a store sized for many batches would launch mostly idle workgroups)
        const bool fused = then_insert && inserted && n_tiles_total && tp.part_end.size() == 1 && !phase_dbg && c->cap && c->own_world <= 1 && !c->lmer_on && !c->routed && !c->pending_m && !prefilter_on(c) &&      // (pre-filter: insertion never rides behind the sketch, the batch is counted first)
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
        if (n_tiles_total) { int e = launch_tiles(c, k, A, init0, tp, sp); if (e) return e; }
        STAGE_EVENT(c, c->ev1, s);                                         // end of the sketch stage = start of the insertion when it rides behind
        if (fused) { int e = launch_fused_insert(c, k); if (e) return e; }
        u64 sc[SC_N];
        int e = read_scalars(c, sc, false, true); if (e) return e;
        c->ms_sketch += ev_ms(c);
        collect_tile_events(c);
        u64 m_new = sc[SC_CARRY];
        const u32 over = (u32)sc[SC_OVERMAX];
        if (over || m_new > c->mcap) {           // a slab or the store was too small: size them from what was seen and run the batch again
            if (over) { sp.slab_cap = std::min<u32>((u32)tile_bases, (over + over / 8 + 15u) & ~7u); c->slab_cap_min = sp.slab_cap; }
            if (m_new > c->mcap) want = m_new + 65536;
            c->n_tile_launches -= tp.part_end.size(); c->n_tile_bases -= n_tiles_total ? n_bases : 0;
            continue;
        }
        if (m_new >= 0xFFFFFFF0ull) return fail(c, MDBG_E_CAPACITY, "more than 2^32 minimizers resident on one device");
        if ((u32)sc[SC_ERRFLAG]) { e = alphabet_rule_pass(c, A, first_ordinal); if (e) return e; }
        const u64 slow_total = sc[SC_SLOWTOTAL];      // (the scalar is scratch from here on)
        if (c->lmer_on && m_new > c->M) { e = lmer_filter_pass(c, k, m_new); if (e) return e; }
        Batch b; b.first_ordinal = first_ordinal; b.n_reads = (u32)n_reads; b.slot0 = slot0; b.m0 = c->M; b.m1 = m_new; b.n_bases = n_bases;
        c->res.invalidate(FROM_UNITIGS);
        if (c->P.flags & MDBG_FLAG_KEEP_READS) { int ke = keep_batch(c, in, d_offsets, n_reads, n_bases, b.kept); if (ke) return ke; }
        store_append(c, b);
        c->n_reads += n_reads; c->n_bases += n_bases; c->n_tiles += n_tiles_total; c->n_slow_tiles += slow_total;
        return fused ? fused_tail(c, sc, inserted) : MDBG_OK;
    }
    return fail(c, MDBG_E_CAPACITY, "minimizer store could not be sized");
}
int sketch_device_impl(mdbg_ctx* c, const u8* d_bases, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 first_ordinal, bool then_insert = false, bool* inserted = nullptr) {
    SketchInput in; in.fmt = FMT_ASCII; in.d_bases = d_bases;
    return sketch_device_impl(c, in, d_offsets, n_reads, n_bases, first_ordinal, then_insert, inserted);
}

// ---- the insertion round ---------------------------------------------------------------------------------------------------------------------------------
// a batch whose windows this rank inserts from the list its sender made (own_lists), without scanning the sketch for them
bool listed(const mdbg_ctx* c, const Batch& b) { return b.list_off != ~0ull && b.owned != ~0ull && c->own_world > 1; }

// SC_BATCHWIN <- exact number of occurrences the round will insert (sizes the table): counted here, unless every batch came with the
// number of its windows this rank owns (counted once by the rank that sketched it: mdbg_owner_counts / mdbg_sketch_commit), whose sum is `known`
int count_round_windows(mdbg_ctx* c, size_t first, size_t last, bool counts_known, u64 known) {
    hipStream_t s = c->stream;
    for (size_t i = first; i < last; ++i) {      // batches that will be scanned (no list, or their windows have to be counted first) need their whole map
        Batch& b = c->batches[i];
        if (!counts_known || !listed(c, b)) fill_mread_of(c, b);
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
    return MDBG_OK;
}
// Dense settings: far more windows than keys.  A table for "every window a new key" would be tens of GB (2 Gbases at the reference CLI's defaults:
// 283 M windows, 19.6 M keys, 13.6 GB), so such rounds go in slices of window starts, each checked on the device against the keys the table holds
// by then; the table grows (doubling) when a slice does not fit and the round resumes at that slice.
int insert_sliced(mdbg_ctx* c, size_t first, size_t last, u64 slice) {
    hipStream_t s = c->stream;
    u32* const flags = (u32*)(scal(c) + SC_CAPERR);                // [0] window index overflow, [1] table too small
    u64 sc[SC_N];
    int e;
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
                                  scal(c) + SC_NWINDOWS, flags, s, nullptr, sl[j].hi - sl[j].a, adm_of(c, b), b.m0);
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
    return close_round(c, sc, TABLE_FULL, 0.0f);                      // (every pass of the loop has added its time)
}
// The insert launches of one plain round over the batches [first, last), back to back: listed batches from their lists, the others by a scan of their sketch
int launch_round_inserts(mdbg_ctx* c, size_t first, size_t last) {
    hipStream_t s = c->stream;
    u32* const flags = (u32*)(scal(c) + SC_CAPERR);
    // a listed batch's pairs and their segments in own_lists; per_entry: launch_insert_listed takes the per-entry kernel for it (the one decision behind the
    // grouping, the claim bytes and the launch below)
    auto list_of = [&](const Batch& b) { return c->own_lists.as<u32>() + b.list_off; };
    auto seg_of = [&](const Batch& b) { return c->own_lists.as<u32>() + b.list_off + 2 * b.owned; };
    auto per_entry = [&](const Batch& b) { return listed_per_entry(table_args(c), b.m0, b.m1, b.owned, seg_of(b) != nullptr); };
    auto shareable = [&](const Batch& b) { return listed(c, b) && b.owned && per_entry(b); };
    // thinly listed batches (a rank's share of the peers' sketches at 4+ ranks) share ONE launch
    std::vector<ListedBatch> multi; u64 multi_total = 0;
    for (size_t i = first; i < last; ++i) {
        const Batch& b = c->batches[i];
        if (shareable(b)) {
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
            if (listed(c, b) && b.m1 > b.m0 && (!b.owned || per_entry(b)))
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
        if (multi_total && shareable(b)) continue;      // went with the shared launch
        if (listed(c, b))          // the sender listed this rank's windows: no scan of the foreign sketch
            launch_insert_listed(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, list_of(b), seg_of(b), b.owned, b.slot0, b.n_reads, b.first_ordinal, flags, s);
        else
            launch_insert_windows(table_args(c), c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, b.slot0, b.first_ordinal,
                                  scal(c) + SC_NWINDOWS, flags, s, nullptr, 0, adm_of(c, b), b.m0);
    }
    return MDBG_OK;
}

// Windows of every resident batch that has not been inserted yet -> counting table.  All pending batches go in one
// round: count their windows, check the capacity rule on the device, launch the inserts back to back, ONE host round
// trip at the end (the insert kernels do nothing if the table has to grow first; then it is grown and the round repeats).
// allow_pending: reserved regions may be waiting for their data (the multi-GPU layer inserts what has landed while the next round
// travels): only committed batches are touched, the regions in flight are not registered yet.
int insert_round_impl(mdbg_ctx* c, bool allow_pending) {
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed) return fail(c, MDBG_E_STATE, "table holds routed records; local insertion is not allowed");
    if (c->pending_m && !allow_pending) return fail(c, MDBG_E_STATE, "reserved sketch regions have not been committed");
    hipStream_t s = c->stream;
    const size_t first = c->batches_inserted, last = c->batches.size();
    c->res.invalidate(FROM_NODES);
    bool any = false;
    for (size_t i = first; i < last; ++i) any = any || c->batches[i].m1 > c->batches[i].m0;
    c->batches_inserted = last;
    if (!any) return MDBG_OK;
    u64 sc[SC_N];
    bool counts_known = c->own_world > 1;
    u64 known = 0;
    for (size_t i = first; i < last; ++i) { const Batch& b = c->batches[i]; if (b.m1 == b.m0) continue; if (b.owned == ~0ull) counts_known = false; else known += b.owned; }
    int e = prefilter_on(c) ? prefilter_admit(c, first, last) : count_round_windows(c, first, last, counts_known, known); if (e) return e;      // (pre-filter: SC_BATCHWIN <- the ADMITTED windows)
    u32* const flags = (u32*)(scal(c) + SC_CAPERR);                // [0] window index overflow, [1] table too small
    u64 total_idx = 0;
    for (size_t i = first; i < last; ++i) total_idx += c->batches[i].m1 - c->batches[i].m0;
    u64 slice = 32ull << 20;
    { const char* sv = getenv("MDBG_INSERT_SLICE"); if (sv) { const u64 v = strtoull(sv, nullptr, 10); if (v) slice = std::max<u64>(v, (u64)OWN_SPAN); } }
    slice = (slice + OWN_SPAN - 1) / OWN_SPAN * OWN_SPAN;
    if (c->own_world <= 1 && total_idx > 2 * slice) return insert_sliced(c, first, last, slice);
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
        e = launch_round_inserts(c, first, last); if (e) return e;
        STAGE_EVENT(c, c->ev1, s);
        if (c->own_world > 1) launch_sum_shards(c->shards.as<u64>() + SH_OWNINS * CTR_SHARDS, 1, scal(c) + SC_OWNINS, s);
        e = read_scalars(c, sc); if (e) return e;
        if (!(sc[SC_CAPERR] >> 32)) break;
        e = table_reserve(c, sc[SC_BATCHWIN]); if (e) return e;          // n_distinct is unchanged: nothing was inserted
    }
    const char* const mismatch = "the owned-window counts passed with the imported sketches do not match their contents";
    if (counts_known && sc[SC_OWNINS] != known) return fail(c, MDBG_E_PARAM, mismatch);
    return close_round(c, sc, mismatch, ev_ms(c));      // (a probe error is reported together with the mismatch)
}
// The insertion of whatever is resident and not in the table.  With the counting pre-filter the round inserts the ADMITTED windows of its batches, and it starts from
// batch 0 whenever a batch has been counted since the round before (prefilter_prepare).
int insert_resident_impl(mdbg_ctx* c, bool allow_pending) {
    if (!prefilter_on(c)) return insert_round_impl(c, allow_pending);
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    if (c->routed || c->own_world > 1 || c->pending_m) return fail(c, MDBG_E_STATE, PF_UNAVAILABLE);
    int e = prefilter_prepare(c); if (e) return e;
    bool any = false;
    for (size_t i = c->batches_inserted; i < c->batches.size(); ++i) any = any || c->batches[i].m1 > c->batches[i].m0;
    const u64 before = c->n_windows;
    e = insert_round_impl(c, allow_pending); if (e) return e;
    if (any) {             // close_round added the round's SC_BATCHWIN, the admitted windows; the round's last read_scalars published SC_NWINDOWS, all windows of its batches
        c->n_windows_admitted += c->n_windows - before;
        c->n_windows = before + c->h_scal[SC_NWINDOWS];
    }
    return MDBG_OK;
}
// What an ingest call does behind its sketch: the batch's windows into the table — or, with the counting pre-filter, into the filter only
int insert_after_sketch(mdbg_ctx* c) { return prefilter_on(c) ? prefilter_count_pending(c) : insert_resident_impl(c); }
}  // namespace

extern "C" {
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
    return inserted ? MDBG_OK : insert_after_sketch(c);
}

// Copies a host batch into a free staging slot (waits for one), WITHOUT the context lock: the copy of one caller overlaps
// the kernels of another.  The slot is released by the StageHold destructor.
struct StageHold {
    mdbg_ctx* c = nullptr; Stage* g = nullptr;
    ~StageHold() { if (g) { { std::lock_guard<std::mutex> l(c->stage_mu); g->busy = false; } c->stage_cv.notify_one(); } }
};
static Stage* acquire_stage(mdbg_ctx* c, StageHold& hold) {
    std::unique_lock<std::mutex> l(c->stage_mu);
    c->stage_cv.wait(l, [&] { return !c->stage[0].busy || !c->stage[1].busy; });
    hold.c = c; hold.g = c->stage[0].busy ? &c->stage[1] : &c->stage[0];
    hold.g->busy = true;
    return hold.g;
}
static int check_host_offsets(mdbg_ctx* c, const uint64_t* offsets, uint64_t n_reads) {
    if (!offsets) return fail(c, MDBG_E_PARAM, "null offsets");
    if (offsets[0] != 0) return fail(c, MDBG_E_PARAM, "offsets[0] must be 0");
    for (u64 r = 0; r < n_reads; ++r) {
        if (offsets[r + 1] < offsets[r]) return fail(c, MDBG_E_PARAM, "offsets must be non-decreasing");
        if (offsets[r + 1] - offsets[r] >= 0xFFFFFFFFull) return fail(c, MDBG_E_CAPACITY, "a read is longer than 2^32-1 bases");
    }
    return MDBG_OK;
}
static int stage_host_batch(mdbg_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, u64* n_bases_out, StageHold& hold) {
    { int e = check_host_offsets(c, offsets, n_reads); if (e) return e; }
    const u64 nb = offsets[n_reads];
    if (nb && !bases) return fail(c, MDBG_E_PARAM, "null bases");
    Stage* g = acquire_stage(c, hold);
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
    return insert_after_sketch(c);
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
    return insert && !inserted ? insert_after_sketch(c) : MDBG_OK;
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
    { int e = check_host_offsets(c, b->offsets, b->n_reads); if (e) return e; }
    const u64 nb = b->offsets[b->n_reads], nw = (nb + 31) / 32;
    if (nb && !b->words) return fail(c, MDBG_E_PARAM, "null packed words");
    for (u64 i = 0; i < b->n_exc; ++i) if (b->exc_pos[i] >= nb || (i && b->exc_pos[i] <= b->exc_pos[i - 1])) return fail(c, MDBG_E_PARAM, "exception positions must be ascending and inside the batch");
    StageHold hold;
    Stage* g = acquire_stage(c, hold);
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
        // sketch into the resident store, copy out; the store is rolled back on every way out of this block
        const StoreRollback tmp(c); const u64 M0 = tmp.s.M;
        const int e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, 0);
        if (e) { if (e == MDBG_E_ALPHABET) c->poisoned = 0; return e; }     // a bad byte in a sketch-only batch does not poison the node table; a device error does
        const u64 m = c->M - M0;
        c->so_hash.resize(m); std::vector<u32> p32(m);
        bool ok = hipStreamSynchronize(c->stream) == hipSuccess;
        if (ok && m) ok = hipMemcpy(c->so_hash.data(), c->mh.as<u64>() + M0, m * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(p32.data(), c->mpos.as<u32>() + M0, m * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) ok = hipMemcpy(c->so_off.data(), c->roff.as<u64>() + c->batches.back().slot0, (n_reads + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess;
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
    if (prefilter_on(c)) { const int e = insert_resident_impl(c); if (e) return e; }      // the table as it stands = the admitted windows of everything resident
    c->q_counts.clear(); c->q_off.assign(n_reads + 1, 0);
    if (n_reads) {
        // sketch into the resident store behind everything that is there, look the windows up; the store is rolled back on every way out of this block
        const StoreRollback tmp(c); const u64 M0 = tmp.s.M;
        const int e = sketch_device_impl(c, hold.g->bases.as<u8>(), hold.g->off.as<u64>(), n_reads, nb, 0);
        if (e) { if (e == MDBG_E_ALPHABET) c->poisoned = 0; return e; }          // a bad byte in a query does not poison the node table; a device error does
        const Batch b = c->batches.back();
        const u64 m = b.m1 - b.m0;
        hipStream_t s = c->stream;
        std::vector<u32> per_min(m);
        std::vector<u64> roffs(n_reads + 1);
        if (m) {
            if (c->q_dev.ensure(m * 4, 0, s) != hipSuccess) return fail(c, MDBG_E_NOMEM, "query buffer");
            launch_query_windows(table_args(c), c->P.min_abundance, c->mh.as<u64>(), c->mread.as<u32>(), c->roff.as<u64>(), b.m0, b.m1, c->q_dev.as<u32>(), s);
            if (hipMemcpyAsync(per_min.data(), c->q_dev.p, m * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return fail(c, MDBG_E_DEVICE, "copy");
        }
        if (hipMemcpyAsync(roffs.data(), c->roff.as<u64>() + b.slot0, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) return fail(c, MDBG_E_DEVICE, "copy");
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
    prefilter_invalidate(c);
    if (new_k == 0) { store_truncate(c, 0); prefilter_drop(c); c->n_tiles = c->n_slow_tiles = 0; return MDBG_OK; }
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
    store_truncate(c, (size_t)mark);
    prefilter_invalidate(c);
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
    o->n_windows_admitted = c->n_windows_admitted; o->prefilter_cells = c->pf_n_cells;
    if (c->link_ctr.p) {
        (void)hipSetDevice(c->dev);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(&o->n_link_matches, c->link_ctr.p, 8, hipMemcpyDeviceToHost));
    }
    return MDBG_OK;
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
