// dist_api.inc — include/mdbg_dist.h: the sketch-exchange multi-GPU mode driven by the library itself (host code; included by
// libmdbg.hip after api.inc).  The same protocol as rust_mdbg_amd/dist.py::ReplicatedMdbg, which stays as the Python test harness.
#include <dlfcn.h>

#include "../../include/mdbg_dist.h"

// ---- RCCL transport, resolved at run time ---------------------------------------------------------------------------------------
namespace {
struct RcclFns {
    // rccl.h:923,933,700,722,678,611 (the prototypes, with ncclComm_t / hipStream_t as opaque pointers and the enums as int)
    int (*GroupStart)();
    int (*GroupEnd)();
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t);
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t);
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t);
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
    bool ok = false;
};
constexpr int NCCL_UINT8 = 1, NCCL_UINT64 = 5, NCCL_SUM = 0;      // ncclDataType_t / ncclRedOp_t (rccl.h)
RcclFns& rccl_fns() {
    static RcclFns f;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = dlopen(nullptr, RTLD_NOW);                        // a host that links (or has loaded) RCCL already: use that copy
        if (!h || !dlsym(h, "ncclGroupStart")) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        f.GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
        f.GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
        f.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
        f.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
        f.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
        f.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
        f.ok = f.GroupStart && f.GroupEnd && f.Send && f.Recv && f.AllGather && f.AllReduce;
    });
    return f;
}
struct RcclComm { void* comm; uint32_t rank, world; hipStream_t st = nullptr; DevBuf d_send, d_recv; };

int rccl_allgather(void* self, const uint64_t* send, uint32_t n, uint64_t* recv) {
    RcclComm* r = (RcclComm*)self; RcclFns& f = rccl_fns();
    if (r->d_send.ensure((size_t)n * 8, 0, r->st) != hipSuccess || r->d_recv.ensure((size_t)n * 8 * r->world, 0, r->st) != hipSuccess) return MDBG_E_NOMEM;
    if (hipMemcpyAsync(r->d_send.p, send, (size_t)n * 8, hipMemcpyHostToDevice, r->st) != hipSuccess) return MDBG_E_DEVICE;
    if (f.AllGather(r->d_send.p, r->d_recv.p, n, NCCL_UINT64, r->comm, r->st) != 0) return MDBG_E_DEVICE;
    if (hipMemcpyAsync(recv, r->d_recv.p, (size_t)n * 8 * r->world, hipMemcpyDeviceToHost, r->st) != hipSuccess) return MDBG_E_DEVICE;
    return hipStreamSynchronize(r->st) == hipSuccess ? MDBG_OK : MDBG_E_DEVICE;
}
// one grouped set of send / recv pairs: each pair of GPUs uses its own xGMI link; messages are cut at 256 MiB (RCCL 2.26 was seen to
// truncate a 1.9 GB message, profiles/r01_notes.md) — both sides cut the same transfer identically
int rccl_exchange_begin(void* self, const mdbg_xfer* sends, uint32_t ns, const mdbg_xfer* recvs, uint32_t nr) {
    RcclComm* r = (RcclComm*)self; RcclFns& f = rccl_fns();
    constexpr uint64_t CUT = 256ull << 20;
    if (f.GroupStart() != 0) return MDBG_E_DEVICE;
    int bad = 0;
    for (uint32_t i = 0; i < nr; ++i) for (uint64_t o = 0; o < recvs[i].bytes; o += CUT)
        bad |= f.Recv((char*)recvs[i].d_ptr + o, (size_t)std::min<uint64_t>(CUT, recvs[i].bytes - o), NCCL_UINT8, (int)recvs[i].peer, r->comm, r->st);
    for (uint32_t i = 0; i < ns; ++i) for (uint64_t o = 0; o < sends[i].bytes; o += CUT)
        bad |= f.Send((const char*)sends[i].d_ptr + o, (size_t)std::min<uint64_t>(CUT, sends[i].bytes - o), NCCL_UINT8, (int)sends[i].peer, r->comm, r->st);
    return f.GroupEnd() != 0 || bad ? MDBG_E_DEVICE : MDBG_OK;          // the transfers run on r->st from here on
}
int rccl_exchange_wait(void* self) { return hipStreamSynchronize(((RcclComm*)self)->st) == hipSuccess ? MDBG_OK : MDBG_E_DEVICE; }
int rccl_exchange(void* self, const mdbg_xfer* sends, uint32_t ns, const mdbg_xfer* recvs, uint32_t nr) {
    const int e = rccl_exchange_begin(self, sends, ns, recvs, nr);
    return e ? e : rccl_exchange_wait(self);
}
int rccl_allreduce(void* self, uint64_t* d_buf, uint64_t n) {
    RcclComm* r = (RcclComm*)self; RcclFns& f = rccl_fns();
    if (!n) return MDBG_OK;
    if (f.AllReduce(d_buf, d_buf, (size_t)n, NCCL_UINT64, NCCL_SUM, r->comm, r->st) != 0) return MDBG_E_DEVICE;
    return hipStreamSynchronize(r->st) == hipSuccess ? MDBG_OK : MDBG_E_DEVICE;
}

// cuts of a batch into C runs of whole reads with roughly equal bases: out[i] = first read of run i (lower bound of the i-th base
// target in the offsets), out[C + 1 + i] = its offset; i = 0 .. C
__global__ void plan_cuts_kernel(const u64* __restrict__ off, u64 n_reads, u32 C, u64* __restrict__ out) {
    const u32 i = threadIdx.x;
    if (i > C) return;
    u64 r = i == C ? n_reads : 0;
    if (i > 0 && i < C) {
        const u64 target = off[0] + (off[n_reads] - off[0]) / C * i;
        u64 lo = 0, hi = n_reads;
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (off[mid] < target) lo = mid + 1; else hi = mid; }
        r = lo;
    }
    out[i] = r; out[C + 1 + i] = off[r];
}
__global__ void rel_offsets_kernel(const u64* __restrict__ abs_off, u64 n, u64 base, u64* __restrict__ rel) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rel[i] = abs_off[i] - base;
}
}  // namespace

struct mdbg_dist {
    mdbg_ctx* ctx = nullptr; mdbg_comm comm{}; RcclComm* own_rccl = nullptr;
    DevBuf rel_off;                              // offsets of my batch relative to its region (what the peers commit)
    std::vector<DevBuf> peer_off, peer_list;     // receive buffers per peer
    // segments (the default exchange): only the hashes the receiver's listed windows need travel (owner.hip, "segments")
    bool settings_checked = false;               // the ranks' versions and settings have been compared (first round)
    bool owner_ready = false; DevBuf own_hist;  // the measured owner table has been built (first round; build_owner_table)
    bool whole = false;                          // mdbg_dist_set_exchange(MDBG_EXCHANGE_WHOLE): ship whole sketches (a later mdbg_dist_reset(k) needs them)
    DevBuf seg_tmp, seg_misc, seg_pay;                            // sender: payload index of every 1,024-entry block of the lists, carry + picks, packed hashes
    DevBuf in_list, in_pay;                                       // receiver: all peers' lists and payloads back to back
    std::vector<uint64_t> pay_base;                               // sender: first payload element of every bucket (+ total)
    std::vector<uint64_t> seg_got;                                // receiver: payload offsets the received lists imply (checked against in_pay_off)
    std::vector<uint64_t> in_list_off, in_pay_off, in_lim;        // receiver: first list entry / payload element of every peer (+ totals); hashes of every peer's sketch
    std::vector<uint64_t> meta, all_meta;
    uint32_t chunks = 1; bool sized = false;     // mdbg_dist_set_pipeline; the store was sized for all chunks of a batch
    DevBuf chunk_off, exc_tmp;                   // offsets (and exception positions) of the chunk being sketched, rebased to its aligned first base
    std::vector<uint64_t> peer_region;           // round in flight: where each peer's sketch lands
    bool in_flight = false, waited = true;
    DevBuf pq_tab, pq_ctr, pq_ord, pq_idx, pq_in, pq_ans_out, pq_ans_in;      // position fetch at finalize (dist_fetch_positions)
    uint64_t bytes_in = 0, bytes_out = 0, fetch_queries = 0;                 // traffic of this rank since create / reset (mdbg_dist_traffic)
    // what every round registered, so that mdbg_dist_reset(new k) can run the rounds again under segments (the resident foreign hashes are the OLD k's):
    // my batch of the round (~0: none) and the batch each peer's sketch became in this context (~0: that peer had nothing)
    struct RoundRec { size_t my_batch; std::vector<size_t> peer_batch; };
    std::vector<RoundRec> rounds; size_t cur_my_batch = ~(size_t)0;
    // host time per stage of the rounds and of finalize, always kept (two clock reads per stage): mdbg_dist_stage_ms hands it out — bench.py puts it into the N > 1 line
    // beside the budget of DESIGN.md 3.4 —, MDBG_DIST_TIMING prints it at destroy
    enum { T_SKETCH, T_WAIT, T_SCATTER, T_COMMIT, T_LISTS, T_PACK, T_GATHER, T_RESERVE, T_SYNC, T_BEGIN, T_INSERT, T_FIN_BEGIN, T_FIN_REDUCE, T_FIN_END, T_FETCH, T_N };
    double t_ms[T_N] = {}; uint64_t n_rounds = 0; bool timing = true, print_timing = getenv("MDBG_DIST_TIMING") != nullptr;
};
static const char* const dist_stage_names[mdbg_dist::T_N] = {"sketch", "wait", "scatter", "commit", "owner_lists", "pack", "allgather", "reserve", "sync", "begin", "insert",
                                                              "finalize_begin", "finalize_allreduce", "finalize_end", "position_fetch"};
struct DistTimer {           // adds the host time of its scope to a stage (the stages end in stream syncs or are host work, so host time is what the step pays)
    mdbg_dist* d; int st; double t0;
    DistTimer(mdbg_dist* d_, int st_) : d(d_), st(st_), t0(d_->timing ? now_ms() : 0.0) {}
    ~DistTimer() { if (d->timing) d->t_ms[st] += now_ms() - t0; }
};

// Called by finalize_end_impl right before fin_emit (through mdbg_ctx::before_emit), on every rank: collective.  See finalize.hip, "positions of
// remote sketches".
static int dist_fetch_positions(void* self, FinArgs& F, u64 n_solid) {
    mdbg_dist* d = (mdbg_dist*)self; mdbg_ctx* c = d->ctx;
    const uint32_t W = d->comm.world, me = d->comm.rank;
    if (W == 1) return MDBG_OK;
    DistTimer tm_fetch(d, mdbg_dist::T_FETCH);              // (inside finalize_end's time)
    hipStream_t s = c->stream;
    // batch -> sketching rank and end of its store region, in F.bt order (fin_setup: batches sorted by first ordinal; the ranges are disjoint)
    std::vector<Batch> bs = c->batches;
    std::sort(bs.begin(), bs.end(), [](const Batch& a, const Batch& b) { return a.first_ordinal < b.first_ordinal; });
    const size_t nb = bs.size();
    std::vector<u64> tab(2 * nb + 1);                       // [nb] m1 (u64) | [nb] src (u32, packed in the tail)
    u32* src_h = (u32*)(tab.data() + nb);
    for (size_t i = 0; i < nb; ++i) { tab[i] = bs[i].m1; src_h[i] = bs[i].src_rank == ~0u ? me : bs[i].src_rank; }
    HIPCHK(c, d->pq_tab.ensure(tab.size() * 8, 0, s));
    HIPCHK(c, hipMemcpyAsync(d->pq_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const u64* m1_dev = d->pq_tab.as<u64>(); const u32* src_dev = (const u32*)(d->pq_tab.as<u64>() + nb);
    HIPCHK(c, d->pq_ctr.ensure((size_t)(3 * W + 1) * 8, 0, s));                    // counts[W] | fill[W] | offs[W] | bad
    HIPCHK(c, hipMemsetAsync(d->pq_ctr.p, 0, (size_t)(3 * W + 1) * 8, s));
    unsigned long long* ctr = (unsigned long long*)d->pq_ctr.p;
    PosQueryArgs Q{}; Q.batch_src = src_dev; Q.me = me; Q.world = W; Q.pass = 0; Q.counts = ctr; Q.fill = ctr + W; Q.offs = (const u64*)(ctr + 2 * W);
    launch_pos_query(F, n_solid, Q, s);
    std::vector<uint64_t> cnt(W, 0), all((size_t)W * W, 0);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), ctr, (size_t)W * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int e = d->comm.allgather_u64(d->comm.self, cnt.data(), W, all.data()); if (e) return fail(c, e, "allgather of the position query counts failed");
    std::vector<uint64_t> off(W + 1, 0), in_off(W + 1, 0);
    for (uint32_t r = 0; r < W; ++r) { off[r + 1] = off[r] + cnt[r]; in_off[r + 1] = in_off[r] + all[(size_t)r * W + me]; }
    const uint64_t n_out = off[W], n_in = in_off[W];
    HIPCHK(c, d->pq_ord.ensure(n_out * 8 + 8, 0, s)); HIPCHK(c, d->pq_idx.ensure(n_out * 8 + 8, 0, s)); HIPCHK(c, d->pq_ans_in.ensure(n_out * 16 + 16, 0, s));
    HIPCHK(c, d->pq_in.ensure(n_in * 8 + 8, 0, s)); HIPCHK(c, d->pq_ans_out.ensure(n_in * 16 + 16, 0, s));
    HIPCHK(c, hipMemcpyAsync(ctr + 2 * W, off.data(), (size_t)W * 8, hipMemcpyHostToDevice, s));
    Q.pass = 1; Q.q_ord = d->pq_ord.as<u64>(); Q.q_idx = d->pq_idx.as<u64>();
    launch_pos_query(F, n_solid, Q, s);
    HIPCHK(c, hipStreamSynchronize(s));                     // the queries are complete before the transport reads them
    std::vector<mdbg_xfer> sends, recvs;
    for (uint32_t r = 0; r < W; ++r) {
        if (r == me) continue;
        if (cnt[r]) sends.push_back({r, d->pq_ord.as<u64>() + off[r], cnt[r] * 8});
        const uint64_t ni = all[(size_t)r * W + me];
        if (ni) recvs.push_back({r, d->pq_in.as<u64>() + in_off[r], ni * 8});
    }
    e = d->comm.exchange(d->comm.self, sends.data(), (uint32_t)sends.size(), recvs.data(), (uint32_t)recvs.size()); if (e) return fail(c, e, "exchange of the position queries failed");
    launch_pos_answer(F, d->pq_in.as<u64>(), n_in, src_dev, me, m1_dev, (uint4*)d->pq_ans_out.p, ctr + 3 * W, s);
    uint64_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, ctr + 3 * W, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    sends.clear(); recvs.clear();
    for (uint32_t r = 0; r < W; ++r) {
        if (r == me) continue;
        const uint64_t ni = all[(size_t)r * W + me];
        if (ni) sends.push_back({r, (uint4*)d->pq_ans_out.p + in_off[r], ni * 16});
        if (cnt[r]) recvs.push_back({r, (uint4*)d->pq_ans_in.p + off[r], cnt[r] * 16});
    }
    e = d->comm.exchange(d->comm.self, sends.data(), (uint32_t)sends.size(), recvs.data(), (uint32_t)recvs.size()); if (e) return fail(c, e, "exchange of the positions failed");
    if (bad) return fail(c, MDBG_E_STATE, "a peer asked for positions of reads this rank did not sketch");
    launch_pos_scatter(d->pq_idx.as<u64>(), (const uint4*)d->pq_ans_in.p, n_out, F.k, c->mpos.as<u32>(), s);
    d->bytes_out += n_out * 8 + n_in * 16; d->bytes_in += n_in * 8 + n_out * 16; d->fetch_queries += n_out;
    return MDBG_OK;
}

extern "C" {

int mdbg_comm_rccl(void* nccl_comm, uint32_t rank, uint32_t world, mdbg_comm* out) {
    if (!nccl_comm || !out || world == 0 || rank >= world) return MDBG_E_PARAM;
    if (!rccl_fns().ok) return MDBG_E_DEVICE;                    // no RCCL in this process and none to load
    RcclComm* r = new RcclComm();
    r->comm = nccl_comm; r->rank = rank; r->world = world;
    if (hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess) { delete r; return MDBG_E_DEVICE; }
    out->self = r; out->rank = rank; out->world = world;
    out->allgather_u64 = rccl_allgather; out->exchange = rccl_exchange; out->allreduce_sum_u64 = rccl_allreduce;
    out->exchange_begin = rccl_exchange_begin; out->exchange_wait = rccl_exchange_wait;
    return MDBG_OK;
}

mdbg_dist* mdbg_dist_create(const mdbg_params* p, const mdbg_comm* comm, int* err) {
    if (!p || !comm || !comm->allgather_u64 || !comm->exchange || !comm->allreduce_sum_u64 || comm->world == 0 || comm->rank >= comm->world ||
        comm->world > OWNL_MAX_WORLD) { if (err) *err = MDBG_E_PARAM; return nullptr; }
    if (p->flags & MDBG_FLAG_PREFILTER) { if (err) *err = MDBG_E_STATE; return nullptr; }      // the counting pre-filter is a one-GPU mode (include/mdbg_hip.h)
    mdbg_ctx* c = mdbg_create(p, err);
    if (!c) return nullptr;
    mdbg_dist* d = new mdbg_dist();
    d->ctx = c; d->comm = *comm;
    if (comm->allgather_u64 == rccl_allgather) d->own_rccl = (RcclComm*)comm->self;
    const int e = mdbg_set_partition(c, comm->world, comm->rank);
    if (e) { if (err) *err = e; mdbg_dist_destroy(d); return nullptr; }
    d->peer_off.resize(comm->world); d->peer_list.resize(comm->world);
    c->before_emit = dist_fetch_positions; c->before_emit_self = d;
    if (err) *err = MDBG_OK;
    return d;
}

void mdbg_dist_destroy(mdbg_dist* d) {
    if (!d) return;
    if (d->print_timing && d->n_rounds) {
        const char* const* nm = dist_stage_names;
        fprintf(stderr, "[mdbg dist timing] rank %u rounds %llu host ms per stage:", d->comm.rank, (unsigned long long)d->n_rounds);
        for (int i = 0; i < mdbg_dist::T_N; ++i) fprintf(stderr, " %s=%.2f", nm[i], d->t_ms[i]);
        fprintf(stderr, "\n");
    }
    if (d->ctx) { (void)hipSetDevice(d->ctx->dev); (void)hipStreamSynchronize(d->ctx->stream); }
    d->peer_off.clear(); d->peer_list.clear(); d->rel_off.release();
    if (d->own_rccl) { if (d->own_rccl->st) (void)hipStreamDestroy(d->own_rccl->st); delete d->own_rccl; }
    if (d->ctx) mdbg_destroy(d->ctx);
    delete d;
}

mdbg_ctx* mdbg_dist_ctx(mdbg_dist* d) { return d ? d->ctx : nullptr; }

// A round = what happens after this rank's batch (if any) has been sketched into the resident store.  round_begin: owner lists, one
// allgather of the sizes, room for the peers' sketches, the grouped exchange is STARTED; round_finish: wait for it, register the
// peers' sketches with the windows this rank owns.  Between the two the caller may sketch its next chunk: the transfers run on the
// transport's own stream.
// First round of an mdbg_dist, before any window is listed (collective): the window minima of this round's batch counted per bin of the value range,
// summed over the ranks, and the bins dealt out heaviest first to the least loaded rank — every rank computes the same table from the same sums
// (integers only).  Bins nobody saw are spread by their index.  See table.hip, OwnerSpec.
static int build_owner_table(mdbg_dist* d, bool have_batch, size_t my_batch) {
    mdbg_ctx* c = d->ctx; hipStream_t s = c->stream;
    const uint32_t W = d->comm.world;
    if (W <= 1 || !owner_bin_mul(c)) { d->owner_ready = true; return MDBG_OK; }          // (the same decision on every rank: it depends on the parameters alone, which the first round has compared)
    HIPCHK(c, d->own_hist.ensure((size_t)OWNER_BINS * 8, 0, s));
    HIPCHK(c, hipMemsetAsync(d->own_hist.p, 0, (size_t)OWNER_BINS * 8, s));
    if (have_batch) { const int e = owner_hist_batch(c, my_batch, d->own_hist.as<u64>()); if (e) return e; }
    HIPCHK(c, hipStreamSynchronize(s));
    int e = d->comm.allreduce_sum_u64(d->comm.self, d->own_hist.as<u64>(), OWNER_BINS); if (e) return fail(c, e, "all-reduce of the window-minimum histogram failed");
    std::vector<uint64_t> h(OWNER_BINS);
    HIPCHK(c, hipMemcpy(h.data(), d->own_hist.p, (size_t)OWNER_BINS * 8, hipMemcpyDeviceToHost));
    // Weight of every bin = a blend of what the first round MEASURED and what a uniform genome would give (the MODEL), the measurement trusted by the share of the
    // model's mass it has seen at all: a representative first round (every heavy bin seen) decides alone, as in rounds 3 - 4; an unrepresentative one (a tiny genome in front
    // of a large one: a few hundred of the heavy bins seen) is mostly overruled — an owner cannot change under a live table, so the first table has to be right for what comes later.
    // Model: the window's smallest hash is the smallest of k draws from the ATOMS, the canonical ntHash values <= bound of the homopolymer-compressed l-mers (no two neighbours
    // equal: 4 x 3^(l-1) strings, enumerated for l <= 14), each as likely as its number of strings: atom j (ascending) is the minimum with probability S_j^k - S_(j+1)^k, S_j = share
    // of the draws >= atom j.  With l = 12 a few hundred atoms carry most windows, which is what made a hash of the value (1.43 at eight ranks), and later a hash of the unseen
    // bins' index (1.28 at four after a skewed first round), lopsided.  Longer l: the atoms are dense, the model is the continuous 1 - (1 - v / bound)^k.
    // Doubles, but every rank runs the same code on the same sums: the same table (ties by bin index).
    std::vector<double> model(OWNER_BINS, 0.0);
    {
        const double bound = owner_hash_bound(c);
        const u64 mul = owner_bin_mul(c);
        const u32 l = c->P.l, k = c->P.k;
        bool enumerated = false;
        if (c->P.scheme == MDBG_SCHEME_DENSITY && l >= 2 && l <= 14) {
            const u64 bnd = bound >= 18446744073709549568.0 ? ~0ull : (u64)bound;
            std::vector<u64> atoms;
            // depth-first over the strings, forward / reverse-complement hashes carried along (bs_core.h seeds; position i contributes rol(h, l-1-i) / rol(rc, i))
            u64 fh[16], rh[16]; int code[16]; int depth = 0;
            fh[0] = rh[0] = 0; code[0] = -1;
            int next[16]; next[0] = 0;
            while (depth >= 0) {
                if (depth == (int)l) { const u64 hmin = fh[depth] < rh[depth] ? fh[depth] : rh[depth]; if (hmin <= bnd) atoms.push_back(hmin); --depth; continue; }
                int cc = next[depth];
                if (depth > 0 && cc == code[depth]) ++cc;              // no two neighbours equal (code[depth] = the base in front)
                if (cc >= 4) { --depth; continue; }
                next[depth] = cc + 1;
                fh[depth + 1] = fh[depth] ^ bs_rol64(bs_seed_f(cc), (unsigned)(l - 1 - depth));
                rh[depth + 1] = rh[depth] ^ bs_rol64(bs_seed_r(cc), (unsigned)depth);
                code[depth + 1] = cc; next[depth + 1] = 0;
                ++depth;
            }
            if (atoms.size() >= 16) {
                std::sort(atoms.begin(), atoms.end());
                const double n = (double)atoms.size();
                size_t j = 0;
                while (j < atoms.size()) {
                    size_t e = j; while (e < atoms.size() && atoms[e] == atoms[j]) ++e;
                    const double s_j = (n - (double)j) / n, s_n = (n - (double)e) / n;
                    const double wgt = pow(s_j, (double)k) - pow(s_n, (double)k);
                    const u64 bin = (u64)(((unsigned __int128)atoms[j] * mul) >> 64);
                    model[bin < OWNER_BINS ? bin : OWNER_BINS - 1] += wgt;
                    j = e;
                }
                enumerated = true;
            }
        }
        if (!enumerated) {
            const double width = (bound + 1.0) / (double)OWNER_BINS;
            double prev = 0.0;
            for (uint32_t i = 0; i < OWNER_BINS; ++i) {
                const double hi = std::min(1.0, ((double)i + 1.0) * width / bound);
                const double f = 1.0 - pow(1.0 - hi, (double)k);
                model[i] = f - prev; prev = f;
            }
        }
    }
    double m_total = 0.0, seen = 0.0;
    for (uint32_t i = 0; i < OWNER_BINS; ++i) { m_total += (double)h[i]; if (h[i]) seen += model[i]; }
    const double trust = m_total > 0.0 ? std::min(1.0, std::max(0.0, seen)) : 0.0;              // share of the model's mass in bins the first round saw
    std::vector<double> wgt(OWNER_BINS);
    for (uint32_t i = 0; i < OWNER_BINS; ++i) wgt[i] = (m_total > 0.0 ? trust * (double)h[i] / m_total : 0.0) + (1.0 - trust) * model[i];
    std::vector<uint32_t> order(OWNER_BINS);
    for (uint32_t i = 0; i < OWNER_BINS; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return wgt[a] != wgt[b] ? wgt[a] > wgt[b] : a < b; });
    std::vector<double> load(W, 0.0);
    std::vector<uint8_t> tab(OWNER_BINS);
    // bins without any weight (nothing measured, no model mass) go by the analytic quantiles of 1 - (1 - v / bound)^k
    std::vector<double> qv(W, 0.0);
    { const double bound = owner_hash_bound(c); for (uint32_t r = 1; r < W; ++r) qv[r] = -expm1(log1p(-(double)r / (double)W) / (double)c->P.k) * bound; }
    const double bin_width = (owner_hash_bound(c) + 1.0) / (double)OWNER_BINS;
    for (uint32_t i : order) {
        if (!(wgt[i] > 0.0)) {
            const double v = ((double)i + 0.5) * bin_width;
            uint32_t r = 0; while (r + 1 < W && qv[r + 1] <= v) ++r;
            tab[i] = (uint8_t)r; continue;
        }
        uint32_t best = 0;
        for (uint32_t r = 1; r < W; ++r) if (load[r] < load[best]) best = r;
        tab[i] = (uint8_t)best; load[best] += wgt[i];
    }
    const int es = owner_set_table(c, W, tab.data());
    if (!es) d->owner_ready = true;              // only a table that is in place counts: a failed first round is tried again by the next one (on every rank: the failure came from a collective)
    return es;
}
// Sender: counts + prefix over the owner lists of my batch (all buckets in one pass), the packed hashes of every bucket, and where each
// bucket's part starts (d->pay_base).  counts[]: entries per bucket, d_lists: the buckets back to back (owner_lists_impl).
static int pack_segments(mdbg_dist* d, const mdbg_batch_info& bi, const uint64_t* counts, const uint32_t* d_lists) {
    mdbg_ctx* c = d->ctx; hipStream_t s = c->stream;
    const uint32_t W = d->comm.world;
    SegBuckets B{}; B.n = W; B.skip = d->comm.rank;             // my own windows' hashes are here already: their bucket is not even in the list (owner_lists_impl, direct_own)
    uint64_t total = 0;
    for (uint32_t r = 0; r < W; ++r) { B.start[r] = total; B.base[r] = bi.store_offset; B.lim[r] = bi.n_minimizers; if (r != d->comm.rank) total += counts[r]; }
    B.start[W] = total;
    d->pay_base.assign(W + 1, 0);
    if (!total) return MDBG_OK;
    HIPCHK(c, d->seg_tmp.ensure((total / 1024 + 2) * 8, 0, s));
    HIPCHK(c, d->seg_misc.ensure((size_t)(OWNL_MAX_WORLD + 4) * 8, 0, s));
    HIPCHK(c, hipMemsetAsync(d->seg_misc.p, 0, 8, s));
    launch_seg_prefix(d_lists, total, c->P.k, B, d->seg_tmp.as<u64>(), d->seg_misc.as<u64>(), d->seg_misc.as<u64>() + 1, s);
    HIPCHK(c, hipMemcpyAsync(d->pay_base.data(), d->seg_misc.as<u64>() + 1, (size_t)(W + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, d->seg_pay.ensure(d->pay_base[W] * 8 + 8, 0, s));
    launch_seg_copy(d_lists, total, c->P.k, B, d->seg_tmp.as<u64>(), c->mh.as<u64>(), d->seg_pay.as<u64>(), d->pay_base[W], false, s);
    return MDBG_OK;
}
// Receiver: the peers' lists and payloads have landed (d->in_list / d->in_pay, peer r at in_list_off[r] / in_pay_off[r]): the hashes go to their
// places in the peers' regions of the store.  A payload that does not match its list's counts is a protocol error.
static int scatter_segments(mdbg_dist* d) {
    mdbg_ctx* c = d->ctx; hipStream_t s = c->stream;
    const uint32_t W = d->comm.world;
    const uint64_t total = d->in_list_off[W];
    if (!total) return MDBG_OK;
    SegBuckets B{}; B.n = W; B.skip = ~0u;
    for (uint32_t r = 0; r < W; ++r) { B.start[r] = d->in_list_off[r]; B.base[r] = d->peer_region[r]; B.lim[r] = d->in_lim[r]; }
    B.start[W] = total;
    HIPCHK(c, d->seg_tmp.ensure((total / 1024 + 2) * 8, 0, s));
    HIPCHK(c, d->seg_misc.ensure((size_t)(OWNL_MAX_WORLD + 4) * 8, 0, s));
    HIPCHK(c, hipMemsetAsync(d->seg_misc.p, 0, 8, s));
    launch_seg_prefix(d->in_list.as<u32>(), total, c->P.k, B, d->seg_tmp.as<u64>(), d->seg_misc.as<u64>(), d->seg_misc.as<u64>() + 1, s);
    // (what the lists imply is compared with what arrived after the round's closing wait for the stream, round_finish: the copy kernel stays inside
    // the payload whatever the lists say — its prefix is checked against the total by seg_copy_kernel's bound)
    d->seg_got.assign(W + 1, 0);
    HIPCHK(c, hipMemcpyAsync(d->seg_got.data(), d->seg_misc.as<u64>() + 1, (size_t)(W + 1) * 8, hipMemcpyDeviceToHost, s));
    launch_seg_copy(d->in_list.as<u32>(), total, c->P.k, B, d->seg_tmp.as<u64>(), c->mh.as<u64>(), d->in_pay.as<u64>(), d->in_pay_off[W], true, s);
    return MDBG_OK;
}
static int round_finish(mdbg_dist* d) {
    if (!d->in_flight) return MDBG_OK;
    mdbg_ctx* c = d->ctx;
    const uint32_t W = d->comm.world, me = d->comm.rank, NM = 3 + 2 * W;
    auto M = [&](uint32_t r, uint32_t f) { return d->all_meta[(size_t)r * NM + f]; };
    if (!d->waited) {
        DistTimer tm(d, mdbg_dist::T_WAIT);
        const int e = d->comm.exchange_wait ? d->comm.exchange_wait(d->comm.self) : MDBG_OK;
        d->waited = true;
        if (e) return fail(c, e, "exchange of sketches failed");
    }
    d->in_flight = false;
    if (!d->whole) { DistTimer tm(d, mdbg_dist::T_SCATTER); const int e = scatter_segments(d); if (e) return e; }
    DistTimer tm_commit(d, mdbg_dist::T_COMMIT);
    mdbg_dist::RoundRec rec; rec.my_batch = d->cur_my_batch; rec.peer_batch.assign(W, ~(size_t)0);
    for (uint32_t r = 0; r < W; ++r) {
        if (r == me) continue;
        const uint32_t* lst = d->whole ? d->peer_list[r].as<u32>() : d->in_list.as<u32>() + 2 * d->in_list_off[r];
        const int e = mdbg_sketch_commit_listed(c, d->peer_region[r], M(r, 0), M(r, 1) ? d->peer_off[r].as<u64>() : nullptr, M(r, 1), M(r, 2),
                                                M(r, 3 + me) ? lst : nullptr, M(r, 3 + me));
        if (e) return e;
        if (M(r, 1)) { c->batches.back().src_rank = r; c->batches.back().partial = !d->whole; rec.peer_batch[r] = c->batches.size() - 1; }      // its positions stayed with rank r (dist_fetch_positions)
    }
    d->rounds.push_back(rec);
    // the receive buffers (offsets, lists) are read by the commits' kernels on the context's stream: the next round may not overwrite them before
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d->whole && d->in_list_off.size() == (size_t)W + 1 && d->in_list_off[W])
        for (uint32_t r = 0; r <= W; ++r) if (d->seg_got[r] != d->in_pay_off[r]) return fail(c, MDBG_E_PARAM, "a peer's packed hashes do not match its window list");
    return MDBG_OK;
}
// my_batch: index of this rank's batch of the round in the context's batch list (~0: the one registered last)
static int round_begin(mdbg_dist* d, bool have_batch, uint32_t rounds_of_batch, size_t my_batch = ~(size_t)0) {
    mdbg_ctx* c = d->ctx;
    const uint32_t W = d->comm.world, me = d->comm.rank;
    (void)hipSetDevice(c->dev);
    hipStream_t s = c->stream;
    // 1. what I have: sizes, ordinal, and the windows of my batch per owning rank (counts + lists)
    const uint32_t NM = 3 + 2 * W;                     // n_minimizers, n_reads, first ordinal | windows per owner | packed hashes per owner
    d->meta.assign(NM, 0); d->all_meta.assign((size_t)NM * W, 0);
    std::vector<uint64_t> counts(W, 0);
    const uint32_t* d_lists = nullptr;
    mdbg_batch_info bi{};
    if (!d->settings_checked) {          // once: every rank runs the same library with the same settings (a mismatch would otherwise surface as a hang or a wrong table)
        // (scheme, syncmer s and the homopolymer flag decide the hash bound the owner function is built from — ranks that differ there would disagree on
        // whether to enter build_owner_table's all-reduce, or build different tables; min_abundance decides which nodes exist)
        constexpr int NS = 10;
        uint64_t dens_bits; { const double dd = c->P.density; memcpy(&dens_bits, &dd, 8); }
        const uint64_t mine[NS] = {MDBG_ABI_VERSION, d->whole ? 1u : 0u, d->chunks, c->P.k, c->P.l, dens_bits, c->P.scheme, c->P.syncmer_s,
                                   (uint64_t)c->P.reads_already_hpc << 32 | c->P.flags, c->P.min_abundance};
        std::vector<uint64_t> all((size_t)NS * W, 0);
        const int e0 = d->comm.allgather_u64(d->comm.self, mine, NS, all.data()); if (e0) return fail(c, e0, "allgather of the ranks' settings failed");
        for (uint32_t r = 0; r < W; ++r) for (int f = 0; f < NS; ++f)
            if (all[(size_t)NS * r + f] != mine[f]) return fail(c, MDBG_E_PARAM, "the ranks differ in library version, exchange mode, chunks per call or sketch parameters (k, l, density, scheme, syncmer s, flags, min_abundance)");
        d->settings_checked = true;
    }
    if (!d->owner_ready) { const int e0 = build_owner_table(d, have_batch, my_batch); if (e0) return e0; }
    ++d->n_rounds;
    d->cur_my_batch = have_batch ? (my_batch == ~(size_t)0 ? c->batches.size() - 1 : my_batch) : ~(size_t)0;
    if (have_batch) {
        int e;
        { DistTimer tm(d, mdbg_dist::T_LISTS); e = owner_lists_impl(c, W, counts.data(), &d_lists, my_batch, true); if (e) return e; }
        e = batch_info_impl(c, &bi, my_batch, false); if (e) return e;          // (pointers only: the stream is waited for once, below, in front of the exchange)
        d->meta[0] = bi.n_minimizers; d->meta[1] = bi.n_reads; d->meta[2] = bi.first_read_ordinal;
        for (uint32_t r = 0; r < W; ++r) d->meta[3 + r] = counts[r];
        if (!d->whole) {
            DistTimer tm(d, mdbg_dist::T_PACK);
            e = pack_segments(d, bi, counts.data(), d_lists); if (e) return e;
            for (uint32_t r = 0; r < W; ++r) d->meta[3 + W + r] = d->pay_base[r + 1] - d->pay_base[r];
        }
    }
    int e;
    { DistTimer tm(d, mdbg_dist::T_GATHER); e = d->comm.allgather_u64(d->comm.self, d->meta.data(), NM, d->all_meta.data()); }
    if (e) return fail(c, e, "allgather of the round's sizes failed");
    std::unique_ptr<DistTimer> tm_reserve(new DistTimer(d, mdbg_dist::T_RESERVE));
    auto M = [&](uint32_t r, uint32_t f) { return d->all_meta[(size_t)r * NM + f]; };
    // 2. room for the peers' sketches at the tail of the resident store: the receives land there directly.  A pipelined batch sizes
    //    the store once for all its chunks (it may not move while a round is in flight)
    uint64_t total_in = 0, all_min = 0, all_reads = 0;
    for (uint32_t r = 0; r < W; ++r) { if (r != me) total_in += M(r, 0); all_min += M(r, 0); all_reads += M(r, 1); }
    if (rounds_of_batch > 1 && !d->sized) {
        e = mdbg_store_reserve(c, c->M + (uint64_t)((double)all_min * rounds_of_batch * 1.2) + (1u << 20), (uint64_t)c->n_slots + (uint64_t)((double)all_reads * rounds_of_batch * 1.2) + 4096ull * rounds_of_batch * W);
        if (e) return e;
        d->sized = true;
    }
    uint64_t* dh = nullptr; uint32_t* dp = nullptr; uint64_t region = 0;
    e = mdbg_sketch_reserve(c, total_in, &dh, &dp, &region); if (e) return e;
    (void)dp;
    if (have_batch) { e = batch_info_impl(c, &bi, my_batch, false); if (e) return e; }          // the reservation may have moved the store: take the pointers now (the stream is waited for below)
    // 3. my offsets relative to my batch (that is how a peer registers them)
    if (have_batch) {
        HIPCHK(c, d->rel_off.ensure((bi.n_reads + 1) * 8, 0, s));
        hipLaunchKernelGGL(rel_offsets_kernel, dim3((unsigned)((bi.n_reads + 256) / 256)), dim3(256), 0, s, bi.d_read_offsets, bi.n_reads + 1, bi.store_offset, d->rel_off.as<u64>());
    }
    std::vector<mdbg_xfer> sends, recvs;
    std::vector<uint64_t> own_base(W + 1, 0);
    for (uint32_t r = 0; r < W; ++r) own_base[r + 1] = own_base[r] + (r == me ? 0 : counts[r]);      // (my own bucket is not in d_lists)
    uint64_t in_off = 0;
    d->peer_region.assign(W, 0);
    d->in_list_off.assign(W + 1, 0); d->in_pay_off.assign(W + 1, 0); d->in_lim.assign(W, 0);
    if (!d->whole) {            // all peers' lists / packed hashes land back to back (one scatter pass over them, round_finish)
        for (uint32_t r = 0; r < W; ++r) {
            const bool in = r != me && M(r, 1);
            d->in_list_off[r + 1] = d->in_list_off[r] + (in ? M(r, 3 + me) : 0);
            d->in_pay_off[r + 1] = d->in_pay_off[r] + (in ? M(r, 3 + W + me) : 0);
            d->in_lim[r] = M(r, 0);
        }
        HIPCHK(c, d->in_list.ensure((d->in_list_off[W] + 1) * 8, 0, s)); HIPCHK(c, d->in_pay.ensure((d->in_pay_off[W] + 1) * 8, 0, s));
    }
    for (uint32_t r = 0; r < W; ++r) {
        if (r == me) continue;
        const uint64_t nm = M(r, 0), nr = M(r, 1), nl = M(r, 3 + me), np = M(r, 3 + W + me);
        d->peer_region[r] = region + in_off;
        if (nr) {
            HIPCHK(c, d->peer_off[r].ensure((nr + 1) * 8, 0, s));
            recvs.push_back({r, d->peer_off[r].p, (nr + 1) * 8});
            if (d->whole) {
                HIPCHK(c, d->peer_list[r].ensure((nl + 1) * 8, 0, s));          // pairs (window, read)
                if (nm) recvs.push_back({r, dh + in_off, nm * 8});          // hashes only: the positions stay with the sketching rank
                if (nl) recvs.push_back({r, d->peer_list[r].p, nl * 8});
                d->bytes_in += nm * 8 + (nr + 1) * 8 + nl * 8;
            } else {
                if (nl) recvs.push_back({r, d->in_list.as<u64>() + d->in_list_off[r], nl * 8});
                if (np) recvs.push_back({r, d->in_pay.as<u64>() + d->in_pay_off[r], np * 8});          // the hashes my windows of its sketch need, nothing else of it
                d->bytes_in += np * 8 + (nr + 1) * 8 + nl * 8;
            }
        }
        in_off += nm;
        if (have_batch && bi.n_reads) {
            sends.push_back({r, d->rel_off.p, (bi.n_reads + 1) * 8});
            if (d->whole) {
                if (bi.n_minimizers) sends.push_back({r, (void*)bi.d_hashes, bi.n_minimizers * 8});
                if (counts[r]) sends.push_back({r, (void*)(d_lists + 2 * own_base[r]), counts[r] * 8});
                d->bytes_out += bi.n_minimizers * 8 + (bi.n_reads + 1) * 8 + counts[r] * 8;
            } else {
                const uint64_t np_out = d->pay_base[r + 1] - d->pay_base[r];
                if (counts[r]) sends.push_back({r, (void*)(d_lists + 2 * own_base[r]), counts[r] * 8});
                if (np_out) sends.push_back({r, d->seg_pay.as<u64>() + d->pay_base[r], np_out * 8});
                d->bytes_out += np_out * 8 + (bi.n_reads + 1) * 8 + counts[r] * 8;
            }
        }
    }
    tm_reserve.reset();
    { DistTimer tm(d, mdbg_dist::T_SYNC); HIPCHK(c, hipStreamSynchronize(s)); }           // my sketch, offsets and lists are complete before the transport reads them
    d->in_flight = true;
    DistTimer tm_begin(d, mdbg_dist::T_BEGIN);
    if (d->comm.exchange_begin && d->comm.exchange_wait) {
        d->waited = false;
        e = d->comm.exchange_begin(d->comm.self, sends.data(), (uint32_t)sends.size(), recvs.data(), (uint32_t)recvs.size());
    } else {
        d->waited = true;
        e = d->comm.exchange(d->comm.self, sends.data(), (uint32_t)sends.size(), recvs.data(), (uint32_t)recvs.size());
    }
    if (e) return fail(c, e, "exchange of sketches failed");
    return MDBG_OK;
}
// one round, not pipelined
static int dist_round(mdbg_dist* d, bool have_batch) {
    MDBG_LOCK(d->ctx);
    int e = round_begin(d, have_batch, 1); if (e) return e;
    e = round_finish(d); if (e) return e;
    return mdbg_insert_resident(d->ctx);
}

// A batch cut into d->chunks runs of whole reads: while chunk c travels to the peers the tile kernel already works on chunk c+1; all
// windows are inserted at the end.  Every rank runs d->chunks rounds, however few reads it holds.
struct ChunkSrc { uint32_t fmt; const uint8_t* d_bases; const mdbg_packed_batch* packed; std::vector<uint64_t> exc_host; DevBuf* exc_tmp; };
static int sketch_chunk(mdbg_dist* d, const ChunkSrc& src, const uint64_t* d_off_chunk, uint64_t n_reads, uint64_t a, uint64_t nb, uint64_t first) {
    if (src.fmt == FMT_ASCII) return mdbg_sketch_device(d->ctx, src.d_bases + a, d_off_chunk, n_reads, nb, first);
    mdbg_packed_batch pb = *src.packed;
    pb.words = (const uint64_t*)((const uint8_t*)src.packed->words + a / 4);           // a is a multiple of 64 bases = 16 bytes of packed words
    pb.offsets = d_off_chunk; pb.n_reads = n_reads;
    if (pb.n_exc) {          // the chunk's slice of the exception list, positions rebased to the chunk's first base
        const uint64_t i0 = (uint64_t)(std::lower_bound(src.exc_host.begin(), src.exc_host.end(), a) - src.exc_host.begin());
        const uint64_t i1 = (uint64_t)(std::lower_bound(src.exc_host.begin(), src.exc_host.end(), a + nb) - src.exc_host.begin());
        pb.n_exc = i1 - i0; pb.exc_val = src.packed->exc_val + i0; pb.exc_pos = nullptr;
        if (pb.n_exc) {
            mdbg_ctx* c = d->ctx;
            HIPCHK(c, src.exc_tmp->ensure(pb.n_exc * 8, 0, c->stream));
            hipLaunchKernelGGL(rel_offsets_kernel, dim3((unsigned)((pb.n_exc + 255) / 256)), dim3(256), 0, c->stream, src.packed->exc_pos + i0, pb.n_exc, a, src.exc_tmp->as<u64>());
            pb.exc_pos = src.exc_tmp->as<u64>();
        }
    }
    return mdbg_sketch_packed_device(d->ctx, &pb, nb, first);
}
static int dist_ingest_chunked(mdbg_dist* d, ChunkSrc& src, const uint64_t* d_offsets, uint64_t n_reads, uint64_t first) {
    mdbg_ctx* c = d->ctx;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    hipStream_t s = c->stream;
    const uint32_t C = d->chunks;
    d->sized = false;                            // the store is sized once per call, for all chunks of this batch
    if (src.fmt == FMT_PLANES && src.packed->n_exc) {
        src.exc_host.resize(src.packed->n_exc);
        HIPCHK(c, hipMemcpyAsync(src.exc_host.data(), src.packed->exc_pos, src.packed->n_exc * 8, hipMemcpyDeviceToHost, s));
    }
    // cuts at read boundaries, roughly equal bases (as rust_mdbg_amd/dist.py::plan_chunks), found on the device: only 2 (C + 1) values come back
    std::vector<uint64_t> cut(C + 1, 0), off_at(C + 1, 0);
    if (n_reads) {
        std::vector<uint64_t> plan(2 * (C + 1));
        HIPCHK(c, d->chunk_off.ensure((size_t)2 * (C + 1) * 8 + 64, 0, s));
        hipLaunchKernelGGL(plan_cuts_kernel, dim3(1), dim3(128), 0, s, d_offsets, n_reads, C, d->chunk_off.as<u64>());
        HIPCHK(c, hipMemcpyAsync(plan.data(), d->chunk_off.p, plan.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (uint32_t i = 0; i <= C; ++i) { cut[i] = plan[i]; off_at[i] = plan[C + 1 + i]; }
        for (uint32_t i = 1; i <= C; ++i) if (cut[i] < cut[i - 1]) { cut[i] = cut[i - 1]; off_at[i] = off_at[i - 1]; }
    }
    for (uint32_t i = 0; i < C; ++i) {
        const uint64_t r0 = cut[i], r1 = cut[i + 1];
        size_t my_batch = ~(size_t)0;
        if (r1 > r0) {
            const uint64_t a = off_at[i] / 64 * 64, nb = off_at[i + 1] - a;         // the chunk starts at an aligned base in front of its first read
            HIPCHK(c, d->chunk_off.ensure((r1 - r0 + 1) * 8, 0, s));
            hipLaunchKernelGGL(rel_offsets_kernel, dim3((unsigned)((r1 - r0 + 256) / 256)), dim3(256), 0, s, d_offsets + r0, r1 - r0 + 1, a, d->chunk_off.as<u64>());
            int e; { DistTimer tm(d, mdbg_dist::T_SKETCH); e = sketch_chunk(d, src, d->chunk_off.as<u64>(), r1 - r0, a, nb, first + r0); }
            if (e == MDBG_E_STATE && d->in_flight) {            // the store would have to grow under the round in flight: finish that first
                e = round_finish(d); if (e) return e;
                e = sketch_chunk(d, src, d->chunk_off.as<u64>(), r1 - r0, a, nb, first + r0);
            }
            if (e) return e;
            my_batch = c->batches.size() - 1;                   // the peers' batches of the round in flight are registered after it
        }
        int e = round_finish(d); if (e) return e;               // chunk i-1 has travelled while chunk i was sketched
        e = round_begin(d, r1 > r0, C, my_batch); if (e) return e;
        // the windows of everything that has landed so far (round i-1 of every rank, my chunk i) go into the table while round i travels
        if (i > 0) { DistTimer tm(d, mdbg_dist::T_INSERT); e = insert_resident_impl(c, true); if (e) return e; }
    }
    int e = round_finish(d); if (e) return e;
    DistTimer tm(d, mdbg_dist::T_INSERT);
    return mdbg_insert_resident(c);
}

int mdbg_dist_set_exchange(mdbg_dist* d, uint32_t mode) {
    if (!d || mode > MDBG_EXCHANGE_WHOLE) return MDBG_E_PARAM;
    if (d->in_flight) return MDBG_E_STATE;
    d->whole = mode == MDBG_EXCHANGE_WHOLE; d->settings_checked = false;
    return MDBG_OK;
}

int mdbg_dist_set_pipeline(mdbg_dist* d, uint32_t chunks) {
    if (!d || chunks < 1 || chunks > 64) return MDBG_E_PARAM;
    d->chunks = chunks; d->settings_checked = false;
    return MDBG_OK;
}

int mdbg_dist_ingest_batch_device(mdbg_dist* d, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!d) return MDBG_E_PARAM;
    if (d->chunks > 1) { if (n_reads && (!d_bases || !d_offsets)) return MDBG_E_PARAM; ChunkSrc src{FMT_ASCII, d_bases, nullptr, {}, &d->exc_tmp}; return dist_ingest_chunked(d, src, d_offsets, n_reads, first_read_ordinal); }
    if (n_reads) { int e = mdbg_sketch_device(d->ctx, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal); if (e) return e; }
    return dist_round(d, n_reads != 0);
}
int mdbg_dist_ingest_batch_packed_device(mdbg_dist* d, const mdbg_packed_batch* batch, uint64_t n_bases, uint64_t first_read_ordinal) {
    if (!d || !batch) return MDBG_E_PARAM;
    if (d->chunks > 1) { if (batch->n_reads && (!batch->words || !batch->offsets)) return MDBG_E_PARAM; ChunkSrc src{FMT_PLANES, nullptr, batch, {}, &d->exc_tmp}; return dist_ingest_chunked(d, src, batch->offsets, batch->n_reads, first_read_ordinal); }
    if (batch->n_reads) { int e = mdbg_sketch_packed_device(d->ctx, batch, n_bases, first_read_ordinal); if (e) return e; }
    return dist_round(d, batch->n_reads != 0);
}

int mdbg_dist_finalize(mdbg_dist* d, mdbg_nodes* out, const uint64_t** d_row, uint64_t* n_nodes_global) {
    if (!d || !out) return MDBG_E_PARAM;
    mdbg_ctx* c = d->ctx;
    uint64_t *bf = nullptr, *bs = nullptr, nw = 0;
    int e;
    { DistTimer tm(d, mdbg_dist::T_FIN_BEGIN); e = mdbg_finalize_begin(c, &bf, &bs, &nw); if (e) return e; }
    {
        DistTimer tm(d, mdbg_dist::T_FIN_REDUCE);          // (the transport's calls return when the result is in place)
        // every bit is set by exactly one rank (distinct keys have distinct first sightings): the sum is the union
        e = d->comm.allreduce_sum_u64(d->comm.self, bf, nw); if (e) return fail(c, e, "all-reduce of the first-sighting bitmap failed");
        e = d->comm.allreduce_sum_u64(d->comm.self, bs, nw); if (e) return fail(c, e, "all-reduce of the solid bitmap failed");
    }
    DistTimer tm(d, mdbg_dist::T_FIN_END);
    return mdbg_finalize_end(c, out, d_row, n_nodes_global);
}

// host milliseconds per stage of this rank's rounds and finalize calls since create or the last call with reset != 0 (names: mdbg_dist_stage_name)
int mdbg_dist_stage_ms(mdbg_dist* d, double* out, uint32_t n, uint64_t* n_rounds, int reset) {
    if (!d || (!out && n)) return MDBG_E_PARAM;
    for (uint32_t i = 0; i < n; ++i) out[i] = i < (uint32_t)mdbg_dist::T_N ? d->t_ms[i] : 0.0;
    if (n_rounds) *n_rounds = d->n_rounds;
    if (reset) { for (double& t : d->t_ms) t = 0; d->n_rounds = 0; }
    return MDBG_OK;
}
const char* mdbg_dist_stage_name(uint32_t i) { return i < (uint32_t)mdbg_dist::T_N ? dist_stage_names[i] : nullptr; }

// Another k under SEGMENTS (collective): a rank holds, of a foreign sketch, only the hashes its windows of the OLD k needed, and with another k both the windows and
// their owners change (the owner is a function of the smallest of the window's k hashes: a k'-window inside a k-window of mine may belong to somebody else, and the
// other way round — no subset relation either way).  So the rounds are run again for the new k from the sketches every rank still holds of its OWN reads: new owner
// lists, new segments into the SAME regions of the store, new window lists for the foreign batches; the reads are not sketched again and nothing of the batch table
// moves.  (After a whole-sketch exchange every hash is resident and mdbg_reset alone does it: one exchange for a sweep of seven k; see bench.py --multik.)
static int dist_reexchange(mdbg_dist* d, uint32_t new_k) {
    mdbg_ctx* c = d->ctx;
    MDBG_LOCK(c);
    (void)hipSetDevice(c->dev);
    if (d->in_flight) return fail(c, MDBG_E_STATE, "a round is in flight");
    if (new_k < 2 || new_k > 4096) return fail(c, MDBG_E_PARAM, "bad k");
    if (c->poisoned) return fail(c, MDBG_E_STATE, "context is in an error state");
    const uint32_t W = d->comm.world, me = d->comm.rank, NM = 3 + 2 * W;
    hipStream_t s = c->stream;
    int e = clear_table(c); if (e) return e;
    c->ms_sketch = c->ms_insert = c->ms_finalize = 0; c->ms_tile = 0; c->n_tile_launches = 0; c->n_tile_bases = 0;
    for (Batch& b : c->batches) { b.owned = ~0ull; b.list_off = ~0ull; }
    c->own_lists_n = 0;
    c->P.k = new_k;
    for (const mdbg_dist::RoundRec& rec : d->rounds) {
        d->meta.assign(NM, 0); d->all_meta.assign((size_t)NM * W, 0);
        std::vector<uint64_t> counts(W, 0);
        const uint32_t* d_lists = nullptr;
        mdbg_batch_info bi{};
        const bool have = rec.my_batch != ~(size_t)0;
        if (have) {
            e = owner_lists_impl(c, W, counts.data(), &d_lists, rec.my_batch, true); if (e) return e;
            e = batch_info_impl(c, &bi, rec.my_batch, false); if (e) return e;
            d->meta[0] = bi.n_minimizers; d->meta[1] = bi.n_reads; d->meta[2] = bi.first_read_ordinal;
            for (uint32_t r = 0; r < W; ++r) d->meta[3 + r] = counts[r];
            e = pack_segments(d, bi, counts.data(), d_lists); if (e) return e;
            for (uint32_t r = 0; r < W; ++r) d->meta[3 + W + r] = d->pay_base[r + 1] - d->pay_base[r];
        }
        e = d->comm.allgather_u64(d->comm.self, d->meta.data(), NM, d->all_meta.data()); if (e) return fail(c, e, "allgather of the round's sizes failed");
        auto M = [&](uint32_t r, uint32_t f) { return d->all_meta[(size_t)r * NM + f]; };
        std::vector<uint64_t> own_base(W + 1, 0);
        for (uint32_t r = 0; r < W; ++r) own_base[r + 1] = own_base[r] + (r == me ? 0 : counts[r]);
        d->peer_region.assign(W, 0);
        d->in_list_off.assign(W + 1, 0); d->in_pay_off.assign(W + 1, 0); d->in_lim.assign(W, 0);
        for (uint32_t r = 0; r < W; ++r) {
            const bool in = r != me && M(r, 1);
            if (in && rec.peer_batch[r] == ~(size_t)0) return fail(c, MDBG_E_STATE, "a peer offers a sketch this rank never registered (the ranks' rounds differ)");
            if (in && (c->batches[rec.peer_batch[r]].m1 - c->batches[rec.peer_batch[r]].m0 != M(r, 0) || c->batches[rec.peer_batch[r]].n_reads != M(r, 1)))
                return fail(c, MDBG_E_STATE, "a peer's sketch has another size than the one registered for this round");
            d->in_list_off[r + 1] = d->in_list_off[r] + (in ? M(r, 3 + me) : 0);
            d->in_pay_off[r + 1] = d->in_pay_off[r] + (in ? M(r, 3 + W + me) : 0);
            d->in_lim[r] = M(r, 0);
            if (in) d->peer_region[r] = c->batches[rec.peer_batch[r]].m0;
        }
        HIPCHK(c, d->in_list.ensure((d->in_list_off[W] + 1) * 8, 0, s)); HIPCHK(c, d->in_pay.ensure((d->in_pay_off[W] + 1) * 8, 0, s));
        std::vector<mdbg_xfer> sends, recvs;
        for (uint32_t r = 0; r < W; ++r) {
            if (r == me) continue;
            const uint64_t nl = M(r, 3 + me), np = M(r, 3 + W + me);
            if (M(r, 1)) {
                if (nl) recvs.push_back({r, d->in_list.as<u64>() + d->in_list_off[r], nl * 8});
                if (np) recvs.push_back({r, d->in_pay.as<u64>() + d->in_pay_off[r], np * 8});
                d->bytes_in += np * 8 + nl * 8;
            }
            if (have && bi.n_reads) {
                const uint64_t np_out = d->pay_base[r + 1] - d->pay_base[r];
                if (counts[r]) sends.push_back({r, (void*)(d_lists + 2 * own_base[r]), counts[r] * 8});
                if (np_out) sends.push_back({r, d->seg_pay.as<u64>() + d->pay_base[r], np_out * 8});
                d->bytes_out += np_out * 8 + counts[r] * 8;
            }
        }
        HIPCHK(c, hipStreamSynchronize(s));
        e = d->comm.exchange(d->comm.self, sends.data(), (uint32_t)sends.size(), recvs.data(), (uint32_t)recvs.size()); if (e) return fail(c, e, "exchange of segments failed");
        e = scatter_segments(d); if (e) return e;
        for (uint32_t r = 0; r < W; ++r) {
            if (r == me || !M(r, 1)) continue;
            Batch& pb = c->batches[rec.peer_batch[r]];
            u64 off = 0;
            e = keep_window_list(c, d->in_list.as<u32>() + 2 * d->in_list_off[r], M(r, 3 + me), M(r, 0), &off); if (e) return e;
            pb.list_off = off; pb.owned = M(r, 3 + me);
        }
        HIPCHK(c, hipStreamSynchronize(s));            // the receive buffers are read by the kernels above: the next round overwrites them
        if (d->in_list_off[W]) for (uint32_t r = 0; r <= W; ++r) if (d->seg_got[r] != d->in_pay_off[r]) return fail(c, MDBG_E_PARAM, "a peer's packed hashes do not match its window list");
    }
    return insert_resident_impl(c);
}

int mdbg_dist_reset(mdbg_dist* d, uint32_t new_k) {
    if (!d) return MDBG_E_PARAM;
    if (new_k == 0) { d->bytes_in = d->bytes_out = d->fetch_queries = 0; d->sized = false; d->rounds.clear(); }
    if (new_k != 0 && new_k != d->ctx->P.k && !d->whole && d->comm.world > 1) return dist_reexchange(d, new_k);
    return mdbg_reset(d->ctx, new_k);
}

int mdbg_dist_traffic(mdbg_dist* d, uint64_t* bytes_in, uint64_t* bytes_out, uint64_t* position_queries) {
    if (!d) return MDBG_E_PARAM;
    if (bytes_in) *bytes_in = d->bytes_in;
    if (bytes_out) *bytes_out = d->bytes_out;
    if (position_queries) *position_queries = d->fetch_queries;
    return MDBG_OK;
}

}  // extern "C"
