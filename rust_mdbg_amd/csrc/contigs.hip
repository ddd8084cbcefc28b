// contigs.hip — contig sequences stitched on the GPU from the resident read store (mdbg_graph_contigs, include/mdbg_hip.h).
//
// The copy plan of a unitig list (unitigs.hip: bases [src_begin, src_begin + len) of read src_read go to [dst_offset, dst_offset + len) of the unitig, through
// utils::revcomp `revcomp` times) is executed against the reads a MDBG_FLAG_KEEP_READS context kept packed 2 bits per base, byte for byte as
// mdbg_emit_contigs_add_batch (mdbg_emit.cpp) executes it against the ASCII reads on the host.
//
// Shape: a pure gather, output-centric.  One thread owns 16 consecutive output bytes and writes them with one 16-byte store.  It finds its contig by binary
// search in the contigs' offsets, its plan entry by binary search in the unitig's dst_offset[], the kept batch of the entry's read by binary search in the batch
// table (all three tables are small next to the output and stay in L2), then funnel-shifts 16 codes out of the two bit planes — for a reverse complement the
// 16 source positions are taken in one piece, bit-reversed (__brev) and the high plane flipped (the complement of code c is c ^ 2) — and expands them to
// "ACTG"[c].  Bytes outside ACGT live in the batch's exception side-list and are patched in only when the batch has any (a branch that is uniform for all
// threads inside one batch).  A 16-byte group that is not covered by ONE plan entry (an entry boundary, a contig boundary, the tail) takes the per-byte path.
// Nothing is written with atomics except the error flag.
#include <cstring>

#include "contigs.h"
#include "graph_common.h"
#include "kept_gather.h"      // the batch lookup, the 16-code expansion, the exception patch: shared with node_seqs.hip

namespace {

struct StitchArgs {
    const u64* out_off; const u64* unitig; u64 n_contigs, n_bases;                                    // the produced contigs
    const u64* u_off; const u64* src_read; const u64* src_begin; const u32* len; const u8* rc; const u64* dst;      // the plan
    const KeptDesc* tab; u32 n_tab;
    u8* out; u32* err;
};

struct Piece {                     // the plan entry that covers an output position, resolved against the store
    const KeptDesc* d;
    u64 sb;                        // position of the entry's first source base in the batch
    u64 within;                    // the output position's offset inside the entry
    u32 n, rc;                     // the entry's length and its revcomp count
};
// false: no kept base belongs at output position g (no entry covers it, or the entry is in error — the flag is set): the byte is 0, as the host path leaves it
__device__ inline bool piece_of(const StitchArgs& A, u64 g, Piece& P) {
    const u64 c = last_le(A.out_off, 0, A.n_contigs, g);
    const u64 u = A.unitig[c];
    const u64 e0 = A.u_off[u], e1 = A.u_off[u + 1], p = g - A.out_off[c];
    if (e0 >= e1) return false;
    const u64 e = last_le(A.dst, e0, e1, p);
    const u64 d0 = A.dst[e];
    const u32 n = A.len[e];
    if (d0 > p || p - d0 >= n) return false;
    const u64 r = A.src_read[e];
    const KeptDesc* const d = kept_batch_of(A.tab, A.n_tab, r);
    if (!d) { atomicOr(A.err, (u32)ERR_NOT_KEPT); return false; }
    u64 sb;
    if (!kept_span(d, r, A.src_begin[e], n, &sb)) { atomicOr(A.err, (u32)ERR_OUTSIDE); return false; }
    P.d = d; P.sb = sb; P.within = p - d0; P.n = n; P.rc = A.rc[e];
    return true;
}
__global__ __launch_bounds__(256) void stitch_kernel(StitchArgs A) {
    const u64 G = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (G >= A.n_bases) return;
    Piece P;
    const bool have = piece_of(A, G, P);
    if (have && P.n - P.within >= 16) {                    // the whole group comes from one entry (and so lies inside the output)
        const bool rev = P.rc == 1;
        const u64 qs = rev ? P.sb + P.n - 16 - P.within : P.sb + P.within;      // lowest of the 16 source positions
        const uint4 ov = kept_group16(P.d, qs, rev, P.rc);
        *(uint4*)(A.out + G) = ov;
        return;
    }
    // an entry boundary, a contig boundary or the tail of the output inside the group: byte by byte
    for (u32 j = 0; j < 16 && G + j < A.n_bases; ++j) {
        u8 v = 0;
        if (piece_of(A, G + j, P)) {
            const u64 q = P.rc == 1 ? P.sb + P.n - 1 - P.within : P.sb + P.within;
            v = through_revcomp(kept_byte(P.d, q), P.rc);
        }
        A.out[G + j] = v;
    }
}

// flag[u] / slen[u] = 1 / length[u] for the unitigs that are produced; entry U of both = 0 (so that the exclusive scans end with the totals)
__global__ void select_kernel(const u64* __restrict__ length, u64 U, u64 min_len, u64* __restrict__ flag, u64* __restrict__ slen) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > U) return;
    const bool take = u < U && length[u] >= min_len;
    flag[u] = take ? 1 : 0; slen[u] = take ? length[u] : 0;
}
__global__ void scatter_kernel(const u64* __restrict__ length, u64 U, u64 min_len, const u64* __restrict__ cidx, const u64* __restrict__ uoff,
                               u64* __restrict__ out_off, u64* __restrict__ unitig) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > U) return;
    if (u == U) { out_off[cidx[U]] = uoff[U]; return; }
    if (length[u] >= min_len) { out_off[cidx[u]] = uoff[u]; unitig[cidx[u]] = u; }
}

}  // namespace

struct ContigBuffers {
    Buf flag, slen, cidx, uoff, tmp, tab, err;
    Buf bases, offsets, unitig;                      // the result: owned until the next stitch_contigs
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
ContigBuffers* contig_buffers_create() { return new ContigBuffers(); }
void contig_buffers_destroy(ContigBuffers* b) {
    if (!b) return;
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    delete b;
}

hipError_t stitch_contigs(ContigBuffers* B, const UnitigResult& ul, const KeptDesc* tab, uint32_t n_tab, uint64_t min_len, hipStream_t s, ContigResult* out) {
    memset(out, 0, sizeof *out);
    const u64 U = ul.n_unitigs;
    u64 C = 0, NB = 0;
    if (U) {
        GHIP(B->flag.ensure((U + 1) * 8)); GHIP(B->slen.ensure((U + 1) * 8)); GHIP(B->cidx.ensure((U + 1) * 8)); GHIP(B->uoff.ensure((U + 1) * 8));
        hipLaunchKernelGGL(select_kernel, dim3((unsigned)((U + 256) / 256)), dim3(256), 0, s, ul.length, U, min_len, B->flag.as<u64>(), B->slen.as<u64>());
        GHIP(excl_scan(B->tmp, B->flag.as<u64>(), B->cidx.as<u64>(), U + 1, s));
        GHIP(excl_scan(B->tmp, B->slen.as<u64>(), B->uoff.as<u64>(), U + 1, s));
        GHIP(hipMemcpyAsync(&C, B->cidx.as<u64>() + U, 8, hipMemcpyDeviceToHost, s));      // (entry U of both inputs is 0: the last outputs ARE the totals)
        GHIP(hipMemcpyAsync(&NB, B->uoff.as<u64>() + U, 8, hipMemcpyDeviceToHost, s));
        GHIP(hipStreamSynchronize(s));
    }
    GHIP(B->offsets.ensure((C + 1) * 8)); GHIP(B->unitig.ensure(C * 8 + 8)); GHIP(B->bases.ensure(NB + 32)); GHIP(B->err.ensure(8));
    GHIP(hipMemsetAsync(B->err.p, 0, 8, s));
    if (!C) GHIP(hipMemsetAsync(B->offsets.p, 0, 8, s));
    else hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((U + 256) / 256)), dim3(256), 0, s, ul.length, U, min_len, B->cidx.as<u64>(), B->uoff.as<u64>(), B->offsets.as<u64>(), B->unitig.as<u64>());
    if (NB) {
        if (n_tab) {
            GHIP(B->tab.ensure((size_t)n_tab * sizeof(KeptDesc)));
            GHIP(hipMemcpyAsync(B->tab.p, tab, (size_t)n_tab * sizeof(KeptDesc), hipMemcpyHostToDevice, s));
        }
        if (!B->ev0) { GHIP(hipEventCreate(&B->ev0)); GHIP(hipEventCreate(&B->ev1)); }
        StitchArgs A{};
        A.out_off = B->offsets.as<u64>(); A.unitig = B->unitig.as<u64>(); A.n_contigs = C; A.n_bases = NB;
        A.u_off = ul.offsets; A.src_read = ul.src_read; A.src_begin = ul.src_begin; A.len = ul.len; A.rc = ul.revcomp; A.dst = ul.dst_offset;
        A.tab = B->tab.as<KeptDesc>(); A.n_tab = n_tab; A.out = B->bases.as<u8>(); A.err = B->err.as<u32>();
        const u64 groups = (NB + 15) / 16, blocks = (groups + 255) / 256;
        if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
        GHIP(hipEventRecord(B->ev0, s));
        hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A);
        GHIP(hipEventRecord(B->ev1, s));
    }
    u32 err = 0;
    GHIP(hipMemcpyAsync(&err, B->err.p, 4, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));                   // (also: `tab` is the caller's)
    GHIP(hipGetLastError());
    if (NB) { float ms = 0; if (hipEventElapsedTime(&ms, B->ev0, B->ev1) == hipSuccess) out->ms_stitch = ms; else (void)hipGetLastError(); }
    out->n_contigs = C; out->n_bases = NB; out->bases = B->bases.as<u8>(); out->offsets = B->offsets.as<u64>(); out->unitig = B->unitig.as<u64>(); out->err = err;
    return hipSuccess;
}

hipError_t sort_exceptions(ContigBuffers* B, const uint64_t* pos_in, const uint8_t* val_in, uint64_t* pos_out, uint8_t* val_out, uint64_t n, hipStream_t s) {
    return sort_pairs(B->tmp, pos_in, pos_out, val_in, val_out, (size_t)n, 0, 64, s);
}
