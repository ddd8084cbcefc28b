// node_seqs.hip — the sequences of the node table's rows gathered on the GPU from the resident read store (mdbg_graph_node_seqs, include/mdbg_hip.h).
//
// Row i of the node table is bases [src_start[i], src_end[i]) of read src_read[i], reverse-complemented through utils::revcomp when reversed[i] — what
// seqfile_write_part (mdbg_emit.cpp) cuts out of the ASCII reads on the host for the .sequences file.  The rows overlap heavily (consecutive nodes share k - 1
// minimizers), so all of them together are many times the input: they are handed out in chunks of consecutive rows under a byte budget.
//
// Once per node table: the rows' lengths and their exclusive prefix (n + 1 entries, cached).  Per chunk: one thread finds the chunk's end in the prefix and the
// host reads the pair {rows, bases} back; the chunk's offsets are the prefix rebased; then the gather.
//
// The gather is output-centric, like stitch_kernel (contigs.hip), whose helpers it shares (kept_gather.h): one thread owns 16 consecutive output bytes and
// writes them with one 16-byte store.  It finds its row by ONE binary search in the chunk's offsets and the row's batch by the search in the batch table — a row
// IS its own copy-plan entry, so the unitig plan's contig -> entry lookups are not needed.  Rows are kilobases long, so almost every group lies inside one
// row: one thread per group keeps all 64 lanes of a wave storing 1 KiB of consecutive output per instruction whatever the rows' lengths, where one wave per row
// would idle lanes at every row's tail and make the short rows of small k as expensive as long ones.  Only groups that straddle a row boundary or the chunk's
// tail go byte by byte.  Nothing is written with atomics except the error flag.
#include <cstring>

#include "graph_common.h"
#include "kept_gather.h"
#include "node_seqs.h"

namespace {

struct NodeSeqArgs {
    const u64* off; u64 n_rows, n_bases, first_row;                   // the chunk: off[n_rows + 1], off[0] = 0, off[n_rows] = n_bases
    const u64* src_read; const u64* src_start; const u8* reversed;   // the node table's columns (indexed by first_row + j)
    const KeptDesc* tab; u32 n_tab;
    u8* out; u32* err;
};

struct RowPiece { const KeptDesc* d; u64 sb, n; bool rev; };      // row j resolved against the store: its first source base in the batch, its length, its orientation
// false: row j has no kept bases (its read is not kept, or it lies outside its read — the flag is set): its bytes are 0
__device__ inline bool row_piece(const NodeSeqArgs& A, u64 j, RowPiece& P) {
    const u64 i = A.first_row + j, r = A.src_read[i], n = A.off[j + 1] - A.off[j];
    const KeptDesc* const d = kept_batch_of(A.tab, A.n_tab, r);
    if (!d) { atomicOr(A.err, (u32)ERR_NOT_KEPT); return false; }
    u64 sb;
    if (!kept_span(d, r, A.src_start[i], n, &sb)) { atomicOr(A.err, (u32)ERR_OUTSIDE); return false; }
    P.d = d; P.sb = sb; P.n = n; P.rev = A.reversed[i] != 0;
    return true;
}

__global__ __launch_bounds__(256) void node_seq_kernel(NodeSeqArgs A) {
    const u64 G = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (G >= A.n_bases) return;
    u64 j = last_le(A.off, 0, A.n_rows, G);                // off[j] <= G < off[j + 1]: rows of length 0 are stepped over (the LAST of equal offsets is found)
    RowPiece P;
    bool have = row_piece(A, j, P);
    const u64 within = G - A.off[j];
    if (have && P.n - within >= 16) {                      // the whole group comes from one row (and so lies inside the output)
        const u64 qs = P.rev ? P.sb + P.n - 16 - within : P.sb + within;      // lowest of the 16 source positions
        *(uint4*)(A.out + G) = kept_group16(P.d, qs, P.rev, P.rev ? 1u : 0u);
        return;
    }
    // a row boundary or the tail of the chunk inside the group: byte by byte, resolving a row when the group enters it
    for (u32 t = 0; t < 16 && G + t < A.n_bases; ++t) {
        const u64 g = G + t;
        if (g >= A.off[j + 1]) {
            do ++j; while (A.off[j + 1] <= g);             // (g < n_bases = off[n_rows]: the walk ends at a row of the chunk)
            have = row_piece(A, j, P);
        }
        u8 v = 0;
        if (have) {
            const u64 w = g - A.off[j];
            v = through_revcomp(kept_byte(P.d, P.rev ? P.sb + P.n - 1 - w : P.sb + w), P.rev ? 1u : 0u);
        }
        A.out[g] = v;
    }
}

// len[i] = src_end[i] - src_start[i] for i < n, len[n] = 0 (so that the exclusive scan ends with the total); a row that ends before it starts has length 0 and is an error
__global__ void row_len_kernel(const u64* __restrict__ src_start, const u64* __restrict__ src_end, u64 n, u64* __restrict__ len, u32* __restrict__ err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    u64 v = 0;
    if (i < n) { const u64 a = src_start[i], b = src_end[i]; if (b < a) atomicOr(err, (u32)ERR_OUTSIDE); else v = b - a; }
    len[i] = v;
}
// one thread: pair = {n_rows, n_bases} of the chunk that starts at row `first` (< n); the chunk's error flag starts as the table's
__global__ void chunk_end_kernel(const u64* __restrict__ prefix, u64 n, u64 first, u64 max_rows, u64 max_bases, u64* __restrict__ pair, const u32* __restrict__ table_err,
                                 u32* __restrict__ err) {
    if (blockIdx.x || threadIdx.x) return;
    const u64 end_max = max_rows && max_rows < n - first ? first + max_rows : n, base = prefix[first];
    u64 lo = first + 1, hi = end_max + 1;                  // the largest end in [first + 1, end_max] within the budget; first + 1 whatever its size
    if (max_bases) while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (prefix[mid] - base <= max_bases) lo = mid; else hi = mid; }
    else lo = end_max;
    pair[0] = lo - first; pair[1] = prefix[lo] - base;
    *err = *table_err;
}
__global__ void chunk_offsets_kernel(const u64* __restrict__ prefix, u64 first, u64 n_rows, u64* __restrict__ off) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_rows) off[t] = prefix[first + t] - prefix[first];
}

}  // namespace

struct NodeSeqBuffers {
    Buf len, prefix, table_err, tmp;                 // per node table
    Buf pair, tab, err;
    Buf bases, offsets;                              // the result: owned until the next node_seq_chunk
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
NodeSeqBuffers* node_seq_buffers_create() { return new NodeSeqBuffers(); }
void node_seq_buffers_destroy(NodeSeqBuffers* b) {
    if (!b) return;
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    delete b;
}

hipError_t node_seq_prefix(NodeSeqBuffers* B, const NodeSeqRows& rows, hipStream_t s) {
    const u64 n = rows.n;
    GHIP(B->len.ensure((n + 1) * 8)); GHIP(B->prefix.ensure((n + 1) * 8)); GHIP(B->table_err.ensure(8));
    GHIP(hipMemsetAsync(B->table_err.p, 0, 8, s));
    hipLaunchKernelGGL(row_len_kernel, dim3(grid_for(n + 1)), dim3(256), 0, s, rows.src_start, rows.src_end, n, B->len.as<u64>(), B->table_err.as<u32>());
    return excl_scan(B->tmp, B->len.as<u64>(), B->prefix.as<u64>(), n + 1, s);
}

hipError_t node_seq_chunk(NodeSeqBuffers* B, const NodeSeqRows& rows, const KeptDesc* tab, uint32_t n_tab, uint64_t first_row, uint64_t max_rows, uint64_t max_bases,
                          hipStream_t s, NodeSeqResult* out) {
    memset(out, 0, sizeof *out);
    out->first_row = first_row;
    const u64 n = rows.n;
    if (first_row >= n) {                            // behind the table: the empty chunk that ends a caller's loop
        GHIP(B->offsets.ensure(8));
        GHIP(hipMemsetAsync(B->offsets.p, 0, 8, s));
        GHIP(hipStreamSynchronize(s));
        out->bases = B->bases.as<u8>(); out->offsets = B->offsets.as<u64>();
        return hipSuccess;
    }
    GHIP(B->pair.ensure(16)); GHIP(B->err.ensure(8));
    hipLaunchKernelGGL(chunk_end_kernel, dim3(1), dim3(64), 0, s, B->prefix.as<u64>(), n, first_row, max_rows, max_bases, B->pair.as<u64>(), B->table_err.as<u32>(), B->err.as<u32>());
    u64 pair[2] = {0, 0};
    GHIP(hipMemcpyAsync(pair, B->pair.p, 16, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));                   // first of the two waits: the chunk's size sizes its buffers and its launch
    GHIP(hipGetLastError());
    const u64 R = pair[0], NB = pair[1];
    if (R == 0 || R > n - first_row) return hipErrorInvalidValue;
    GHIP(B->offsets.ensure((R + 1) * 8)); GHIP(B->bases.ensure(NB + 32));
    hipLaunchKernelGGL(chunk_offsets_kernel, dim3(grid_for(R + 1)), dim3(256), 0, s, B->prefix.as<u64>(), first_row, R, B->offsets.as<u64>());
    if (NB) {
        if (n_tab) {
            GHIP(B->tab.ensure((size_t)n_tab * sizeof(KeptDesc)));
            GHIP(hipMemcpyAsync(B->tab.p, tab, (size_t)n_tab * sizeof(KeptDesc), hipMemcpyHostToDevice, s));
        }
        if (!B->ev0) { GHIP(hipEventCreate(&B->ev0)); GHIP(hipEventCreate(&B->ev1)); }
        NodeSeqArgs A{};
        A.off = B->offsets.as<u64>(); A.n_rows = R; A.n_bases = NB; A.first_row = first_row;
        A.src_read = rows.src_read; A.src_start = rows.src_start; A.reversed = rows.reversed;
        A.tab = B->tab.as<KeptDesc>(); A.n_tab = n_tab; A.out = B->bases.as<u8>(); A.err = B->err.as<u32>();
        const u64 groups = (NB + 15) / 16, blocks = (groups + 255) / 256;
        if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
        GHIP(hipEventRecord(B->ev0, s));
        hipLaunchKernelGGL(node_seq_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A);
        GHIP(hipEventRecord(B->ev1, s));
    }
    u32 err = 0;
    GHIP(hipMemcpyAsync(&err, B->err.p, 4, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));                   // second wait: the error flag (also: `tab` is the caller's)
    GHIP(hipGetLastError());
    if (NB) { float ms = 0; if (hipEventElapsedTime(&ms, B->ev0, B->ev1) == hipSuccess) out->ms_gather = ms; else (void)hipGetLastError(); }
    out->n_rows = R; out->n_bases = NB; out->bases = B->bases.as<u8>(); out->offsets = B->offsets.as<u64>(); out->err = err;
    return hipSuccess;
}
