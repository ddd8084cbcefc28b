/* mdbg_hip.h — C ABI of libmdbg_hip.so: MI355X-native minimizer sketching + k-min-mer counting.
 *
 * This is the drop-in boundary for rust-mdbg's per-read hot path.  The reference has NO plugin/FFI
 * interface for it (the path is a set of closures inside fn main()), so the boundary is cut along the
 * seams SURVEY.md §8b identifies; each entry point names the reference code it replaces
 * (paths relative to the rust-mdbg tree):
 *
 *   mdbg_create            Params {k,l,density,min_kmer_abundance,reads_already_hpc}   src/main.rs:92-114,515-537
 *                          + dbg_nodes / NODE_INDEX construction                       src/main.rs:595-598
 *   mdbg_ingest_batch      process_read_aux over a batch of records                    src/main.rs:730-785
 *     (= Read::extract_density  src/read.rs:176-211, encode_rle src/read.rs:157-174, nthash::NtHashIterator,
 *        the k-min-mer window loop src/main.rs:756-781, KmerVec::normalize src/kmer_vec.rs:34-39 and
 *        add_kminmer's counting upsert src/main.rs:632-691)
 *   mdbg_ingest_batch_packed   the same over reads packed 2 bits per base by the host (mdbg_pack_reads of mdbg_emit.h), replacing
 *                          the per-read String copies of src/main.rs:733-739: a quarter of the bytes over PCIe and through HBM
 *   mdbg_sketch_only       Read::extract (density scheme)                              src/read.rs:85-90,176-211
 *   mdbg_finalize          abundance filter + read-only view of dbg_nodes              src/main.rs:922-929,1014-1016
 *                          + what the .sequences line of a node is built from          src/main.rs:693-708
 *   mdbg_graph_edges       km_index + orientation tests + presimp + overlaps           src/main.rs:1017-1117
 *   mdbg_query_batch       --read_stats: abundance of every k-min-mer of a query read  src/main.rs:939-1004
 *   mdbg_reset             a new k over the same reads (utils/multik:69-78 re-runs the binary per k)
 *   mdbg_set_lmer_filter   --lmer-counts: restrict the minimizers to the l-mers selected from a counts file
 *   mdbg_mark / _rewind    ... with the script's contig feedback: forget the last round's contigs, keep the reads' sketches
 *   mdbg_destroy           process exit
 *
 * Conventions: every function returns 0 (MDBG_OK) or a negative error code and never aborts (the reference
 * panics); strings are (ptr,len); the caller owns its input buffers and may free them when a call returns;
 * the library owns the context and every buffer it hands out until the next call that documents otherwise
 * or mdbg_destroy.  Semantics are those of the reference run with `--threads 1` and without `--bf`
 * (MDBG_FLAG_PREFILTER is this library's order-free counterpart of `--bf`, defined at the flag):
 * results do not depend on how reads are split into batches or on the order of the calls, only on
 * `first_read_ordinal` (the position of the batch's first record in the input file).
 *
 * No torch / HIP types appear here: device buffers are plain pointers.
 */
#ifndef MDBG_HIP_H
#define MDBG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDBG_ABI_VERSION 3      /* 3: the owner of a k-min-mer is a function of its smallest hash (ranks of a multi-GPU job must run the same version) */

enum {
    MDBG_OK = 0,
    MDBG_E_PARAM = -1,    /* bad parameter (k<2, l out of range, minabund==0, null pointer ...) */
    MDBG_E_ALPHABET = -2, /* a read whose HPC length is >= l holds a byte outside "ACGTN" (reference: nthash panics) */
    MDBG_E_CAPACITY = -3, /* a fixed limit was exceeded (e.g. more than 2^26 minimizers in one read) */
    MDBG_E_DEVICE = -4,   /* HIP runtime failure; text via mdbg_last_error */
    MDBG_E_NOMEM = -5,    /* device or host allocation failed */
    MDBG_E_STATE = -6,    /* call not valid in the context's current state (e.g. ingest after an error) */
    MDBG_E_IO = -7        /* libmdbg_emit: a file could not be opened, or a write / close failed (disk full ...) */
};

#define MDBG_MAX_L 255u        /* l = 2..32 run on the bit-sliced kernel, longer l-mers on its generic exact walker (reference: unbounded) */
#define MDBG_MAX_MINABUND 65535u /* DbgAbundance is a u16 in the reference; up to 8 the table tracks the A-th sighting directly, above it is recovered at finalize */
#define MDBG_FLAG_FORCE_GENERIC 1u /* every tile takes the generic exact sketch kernel (testing / cross-check) */
#define MDBG_FLAG_KEEP_READS 2u  /* the context keeps every batch it ingests WITH bases, packed 2 bits per base, in device memory: mdbg_graph_contigs and mdbg_graph_node_seqs gather from that store */
/* MDBG_FLAG_PREFILTER — the counting pre-filter (the reference's --bf, made independent of order).
 *
 * The reference's Bloom filter lets a k-min-mer into dbg_nodes at its second sighting (src/main.rs:632-691, Bloom branch); it is racy under --threads and credits a
 * false positive with abundance 2.  Neither is copied.  A context created with this flag has a filter of n_cells cells, n_cells = mdbg_params.prefilter_cells as
 * given (0: 2^32; 1 <= n_cells <= 2^36, else MDBG_E_PARAM), fixed for the context's life; a cell is a 2-bit counter that saturates at 2 (n_cells / 4 bytes of
 * device memory).  The flag needs min_abundance >= 2 (MDBG_E_PARAM with 1).
 *
 *   Cell of a window:  cell = mulhi64(fmix64(h ^ 0x9E3779B97F4A7C15), n_cells), mulhi64 = the high 64 bits of the 128-bit product,
 *     fmix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33   (all arithmetic mod 2^64),
 *     h = the table's key hash of the window's canonical key c[0 .. k) (KmerVec::normalize: the window, or its reverse when that is the smaller one — ties reversed):
 *       h0 = 0x243F6A8885A308D3, h1 = 0x13198A2E03707344, h2 = 0xA4093822299F31D0, h3 = 0x082EFA98EC4E6C89;
 *       for j = 0 .. k-1 in order, with i = j mod 4:   hi = (hi ^ c[j]) * 0x9E3779B97F4A7C15;  hi ^= hi >> 29;
 *       h = fmix64(h0 ^ rol64(h1, 17) ^ rol64(h2, 31) ^ rol64(h3, 47))                          (rol64: rotate left).
 *   Cell value:  after counting, min(2, number of window occurrences among ALL resident batches whose key maps to the cell).
 *   Admission:  a window is admitted iff its cell value is 2, and the table holds exactly the admitted windows, with their true ordinals.  So every key seen at
 *     least twice is in the table with its exact count, first sighting and A-th sighting; a key seen once is in the table, with count 1, iff it shares its cell
 *     with another occurrence (of any key).
 *   Node table:  for min_abundance >= 2 the table of mdbg_finalize* has the same rows in the same order as without the flag; n, keys, abundance, seqlen, shift,
 *     shift_full, src_read, src_start, src_end, reversed and n_wrapped are bit-identical.  `index` is the rank of the first sighting among the keys the TABLE
 *     holds (strictly increasing, <= the exact value) and n_distinct is the number of keys the table holds.  With n_cells == 1 and at least two windows everything
 *     is admitted and the whole result equals the exact mode's.  Like the exact mode, results depend on the reads, their ordinals and the parameters only — never
 *     on the batch split, the call order or finalizes in between.
 *   How it runs:  the ingest calls sketch the batch and count its windows into the filter; nothing is inserted.  The admitted windows are inserted at the start
 *     of every call that reads the table (mdbg_insert_resident, mdbg_finalize*, mdbg_query_batch; the graph stages read the last finalize's table).  Windows of
 *     earlier batches can become admissible through a later batch, so when a batch was counted since the last insertion and the table is not empty, the table is
 *     cleared and EVERY resident batch is inserted again: alternating ingest and finalize re-inserts.  mdbg_reset(new_k) and mdbg_rewind make the filter stale
 *     (counts cannot be taken back): it is zeroed and every resident batch counted again; mdbg_reset(ctx, 0) drops it.
 *   Not available (MDBG_E_STATE): mdbg_set_partition with world > 1, mdbg_route_pack / mdbg_insert_records / mdbg_routed_export, and the mdbg_dist_* layer
 *     (mdbg_dist_create).
 *   mdbg_stats: n_windows_admitted, prefilter_cells. */
#define MDBG_FLAG_PREFILTER 4u
#define MDBG_SCHEME_DENSITY 0u  /* canonical ntHash <= density * 2^64           Read::extract_density   src/read.rs:176-211 */
#define MDBG_SCHEME_SYNCMERS 1u  /* --syncmers: open syncmers (smallest s-mer in the middle), down-sampled by hash(l-mer) <= density * 4^l;
                                  * 2-bit codes, A/a C/c G/g T/t/U/u, any other byte resets (no alphabet error); l <= 31
                                  *                                              Read::extract_syncmers  src/read.rs:215-352 */

typedef struct mdbg_ctx mdbg_ctx;

/* src/main.rs:92-114 (the fields this path reads) */
typedef struct mdbg_params {
    uint32_t k;                 /* k-min-mer length, >= 2                                   (-k) */
    uint32_t l;                 /* minimizer length, 2..MDBG_MAX_L                          (-l) */
    double density;             /* hash_bound = floor(density * 2^64), src/read.rs:183      (--density) */
    uint32_t min_abundance;     /* 1..MDBG_MAX_MINABUND                                     (--minabund) */
    uint32_t reads_already_hpc; /* nonzero: skip homopolymer compression                    (--skiphpc) */
    int32_t device;             /* HIP device ordinal, -1 = current device */
    uint32_t flags;             /* MDBG_FLAG_* */
    uint64_t table_capacity_hint; /* expected number of distinct k-min-mers, 0 = size from the data */
    uint32_t scheme;            /* MDBG_SCHEME_*: how minimizers are selected (Read::extract, src/read.rs:85-90) */
    uint32_t syncmer_s;         /* MDBG_SCHEME_SYNCMERS: s-mer length, 0..min(l, 16) with l - s + 1 <= 32 (-s, default 4 in the reference) */
    uint64_t prefilter_cells;   /* MDBG_FLAG_PREFILTER: number of cells of the counting pre-filter, 1 .. 2^36; 0 = the default 2^32 (1 GiB)  (--bf) */
    uint64_t reserved[2];
} mdbg_params;

/* Read-only view of the abundance-filtered node table (what src/main.rs:1014-1117 iterates).
 * Nodes are sorted by `index`.  All arrays are library-owned HOST memory, valid until the next
 * mdbg_finalize / mdbg_reset / mdbg_destroy on the context. */
typedef struct mdbg_nodes {
    uint64_t n;                 /* number of nodes after the abundance filter (main.rs:927) */
    uint32_t k;
    const uint64_t* keys;       /* n*k : canonical k-min-mer (KmerVec::normalize().0) */
    const uint32_t* index;      /* n   : DbgEntry.index = rank of first sighting among ALL distinct k-min-mers (NODE_INDEX) */
    const uint16_t* abundance;  /* n   : DbgEntry.abundance (u16, wraps like the reference) */
    const uint32_t* seqlen;     /* n   : DbgEntry.seqlen of the A-th sighting (main.rs:680-682,778; see n_wrapped) */
    const uint16_t* shift;      /* n*2 : DbgEntry.shift, truncated to u16 (main.rs:675) */
    const uint64_t* shift_full; /* n*2 : un-truncated shift as printed in the .sequences line (main.rs:702) */
    const uint64_t* src_read;   /* n   : ordinal of the read the A-th sighting came from */
    const uint64_t* src_start;  /* n   : raw offset of the node's sequence in that read  (read_offsets.0) */
    const uint64_t* src_end;    /* n   : raw end (exclusive) = pos[i+k-1] + l              (read_offsets.1) */
    const uint8_t* reversed;    /* n   : seq_reversed of that sighting (sequence must be reverse-complemented, main.rs:701) */
    uint64_t n_distinct;        /* "Number of nodes before abundance filter" (main.rs:926) */
    uint64_t n_wrapped;         /* nodes seen >= 65536 times: the abundance wrapped like the reference's u16, and seqlen / shift / src_*
                                 * are those of sighting A + 65536*floor((count-A)/65536): the reference refreshes the entry whenever
                                 * the abundance before the increment equals A-1 (main.rs:676-684) */
} mdbg_nodes;

typedef struct mdbg_stats {
    uint64_t n_reads, n_bases, n_minimizers, n_windows, n_distinct, table_capacity;
    uint64_t n_slow_tiles;      /* tiles that took the generic exact walker (a byte outside ACGT, or > 200 bases of one homopolymer in front of the tile) */
    uint64_t n_tiles;
    double ms_sketch, ms_insert, ms_finalize; /* device time (HIP events) accumulated over calls since create/reset */
    double ms_sketch_tile;      /* of ms_sketch: time inside sketch_tile_kernel launches only (HIP events around each launch) */
    uint64_t n_sketch_tile_launches;
    uint64_t n_sketch_tile_bases; /* raw bases covered by those launches */
    uint64_t tile_bases;        /* raw bases a tile owns under this context's parameters (n_tiles = sum over batches of ceil(batch bases / tile_bases)) */
    uint64_t n_link_matches;    /* only with MDBG_COUNT_LINKS in the environment (test hook; 0 otherwise): repeats of a key confirmed as a LINK of their left neighbour's
                                 * match (one value compared instead of k: csrc/table.hip, upsert_wave), since create / mdbg_reset */
    uint64_t n_windows_admitted; /* MDBG_FLAG_PREFILTER: windows the pre-filter let into the table (n_windows stays the number of windows of the ingested reads); 0 without the flag */
    uint64_t prefilter_cells;   /* MDBG_FLAG_PREFILTER: the number of cells in force; 0 without the flag */
    uint64_t reserved[1];
} mdbg_stats;

mdbg_ctx* mdbg_create(const mdbg_params* p, int* err);
void mdbg_destroy(mdbg_ctx* ctx);

/* Threading: every entry point may be called from any host thread; calls on one context are serialised internally.
 * mdbg_ingest_batch (and mdbg_sketch_only) may be called CONCURRENTLY from several threads, as the reference calls
 * process_read_aux from its --threads workers (src/main.rs:834-913): each caller's PCIe copy runs in its own staging
 * slot and overlaps the kernels of the others.  Batches are ordered by first_read_ordinal, not by call time, so the node
 * table does not depend on the interleaving.  Result buffers (mdbg_sketch_only, mdbg_finalize) belong to the context:
 * callers that need them concurrently use one context each.  mdbg_destroy must not race with other calls.
 *
 * Ingest a batch of reads given as concatenated ASCII (HOST memory) + n_reads+1 offsets.  The bytes are
 * copied to the device and processed there; the sketch of every read stays resident for mdbg_reset. */
int mdbg_ingest_batch(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                      uint64_t first_read_ordinal);
/* Same, with both buffers already in DEVICE memory (d_bases 16-byte aligned).  n_bases = offsets[n_reads].
 * offsets[0] may be > 0: bytes in front of the first read are ignored (lets a caller pass an aligned pointer into the
 * middle of a larger buffer). */
int mdbg_ingest_batch_device(mdbg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads,
                             uint64_t n_bases, uint64_t first_read_ordinal);

/* ---- 2-bit packed input -------------------------------------------------------------------------------------
 * Layout: one uint64_t per 32 bases of the concatenated batch, word w = bases [32w, 32w + 32): bit i (0..31) = bit 1 of the
 * ASCII byte of base 32w + i, bit 32 + i = bit 2 of that byte, i.e. the two bits of the code (ascii >> 1) & 3 (A=0 C=1 T=2
 * G=3) as two 32-bit planes.  Bits past the last base are ignored.  Every byte that is not one of "ACGT" (N, lower case,
 * anything else) is listed in the exception side-list (position in the batch ascending, original byte); its two bits in
 * the words are ignored.  The GPU kernel reads the planes as they are (no unpacking step) and treats tiles that hold an
 * exception with the generic exact walker, so N hashes as 0 and other bytes raise MDBG_E_ALPHABET under the reference's
 * rule, exactly as with ASCII input.  mdbg_pack_reads (mdbg_emit.h, host) and mdbg_pack_device (below) produce the layout. */
typedef struct mdbg_packed_batch {
    const uint64_t* words;      /* (n_bases + 31) / 32 words, 16-byte aligned when in device memory */
    const uint64_t* offsets;    /* n_reads + 1 offsets in BASES into the concatenated batch */
    uint64_t n_reads;
    const uint64_t* exc_pos;    /* n_exc positions, ascending */
    const uint8_t* exc_val;     /* n_exc bytes */
    uint64_t n_exc;
} mdbg_packed_batch;
/* HOST buffers (offsets[0] must be 0); same semantics and thread-safety as mdbg_ingest_batch. */
int mdbg_ingest_batch_packed(mdbg_ctx* ctx, const mdbg_packed_batch* batch, uint64_t first_read_ordinal);
/* DEVICE buffers; n_bases = offsets[n_reads].  _sketch_ runs the sketch stage only (see mdbg_sketch_device). */
int mdbg_ingest_batch_packed_device(mdbg_ctx* ctx, const mdbg_packed_batch* batch, uint64_t n_bases, uint64_t first_read_ordinal);
int mdbg_sketch_packed_device(mdbg_ctx* ctx, const mdbg_packed_batch* batch, uint64_t n_bases, uint64_t first_read_ordinal);
/* ASCII -> packed on the device (DEVICE buffers; d_words holds (n_bases + 31) / 32 words).  Exceptions are appended to
 * d_exc_pos / d_exc_val (room for exc_cap entries, sorted by position on return); *n_exc is their number — if it exceeds
 * exc_cap the lists are incomplete and the call returns MDBG_E_CAPACITY. */
int mdbg_pack_device(mdbg_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, uint64_t* d_words, uint64_t* d_exc_pos,
                     uint8_t* d_exc_val, uint64_t exc_cap, uint64_t* n_exc);

/* The Read::extract seam alone: sketches a batch (HOST buffers) without touching the node table.
 * Outputs (library-owned host memory, valid until the next call on ctx): hashes[m] = Read.transformed,
 * positions[m] = Read.minimizers_pos, per_read_offsets[n_reads+1] delimiting each read's slice. */
int mdbg_sketch_only(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                     const uint64_t** hashes, const uint64_t** positions, const uint64_t** per_read_offsets,
                     uint64_t* n_minimizers);

/* --read_stats (src/main.rs:939-1004, src/read_stats.rs): for every read of the batch (HOST buffers, as mdbg_ingest_batch) and every
 * k-min-mer window of it (reads with MORE than k minimizers only), the abundance of that k-min-mer in the table as it stands after the
 * abundance filter: DbgEntry.abundance (u16) of a node that passes --minabund, else 0.  counts[per_read_offsets[r] ..
 * per_read_offsets[r+1]) are the values of read r in window order - one ".read_stats" line "{id}: c0 c1 ... ".  The batch is sketched
 * on the device and looked up there; neither the table nor the resident sketches change.  Library-owned HOST arrays, valid until the
 * next call on ctx.  Not available on a context that holds routed records. */
int mdbg_query_batch(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, const uint32_t** counts,
                     const uint64_t** per_read_offsets, uint64_t* n_windows);

/* The node table of every batch ingested so far (HOST arrays owned by the context, valid until the next call on ctx).  mdbg_finalize and the ingest calls may
 * alternate, with the batches' first_read_ordinal in any order: each finalize describes all batches ingested so far, as if they had arrived in ordinal order. */
int mdbg_finalize(mdbg_ctx* ctx, mdbg_nodes* out);
/* Same node table, but every pointer in *out is DEVICE memory (no copy to the host). */
int mdbg_finalize_device(mdbg_ctx* ctx, mdbg_nodes* out);
/* The node table for a host that writes the .gfa and nothing else: it stays on the device (where mdbg_graph_edges reads it), and only what the S lines print
 * comes to the host — out->index, out->seqlen, out->abundance (HOST arrays: 10 bytes per node instead of 8 k + 58); every other pointer of *out is NULL.
 * mdbg_emit_write_gfa accepts such a table, the .sequences writer and mdbg_emit_edges do not (they need the minimizer lists: MDBG_E_PARAM). */
int mdbg_finalize_gfa(mdbg_ctx* ctx, mdbg_nodes* out);
/* Order-free digest of a node table whose arrays are in DEVICE memory (mdbg_finalize_device, mdbg_dist_finalize): per node
 *   h = 0x243F6A8885A308D3 ^ abundance;  h = fmix64(h ^ key[j]) for j = 0 .. k-1     (fmix64: the 64-bit finaliser of MurmurHash3)
 * *sum = the sum of h over the nodes mod 2^64, *xr = their XOR.  Equal digests and node counts: the same set of (key, abundance) pairs, i.e. what
 * dbg_nodes holds after the abundance filter (src/main.rs:922-929), whatever the order of the rows; the digests of the ranks' partitions of a multi-GPU
 * run add / XOR up to the digest of the one-GPU table.  Only nodes->n, k, keys, abundance are read.  (bench.py compares it with the CPU oracle's digest
 * of the same reads in every run: a full-size check of the node SET, not of two counts.) */
int mdbg_nodes_digest(mdbg_ctx* ctx, const mdbg_nodes* nodes, uint64_t* sum, uint64_t* xr);
/* Multi-k: keep every cached sketch and all allocations, clear the node table, and re-window the
 * resident sketches with new_k (new_k == 0: also drop the sketches = start over with the same parameters). */
int mdbg_reset(mdbg_ctx* ctx, uint32_t new_k);
/* --lmer-counts (robust minimizers; src/main.rs:544-575, src/minimizers.rs:53-113, src/read.rs:200-205): a minimizer that passed the density
 * threshold is kept only if its l-mer is one of the SELECTED l-mers of a counts file.  codes: the selected l-mers, BOTH orientations
 * listed (the reference inserts an l-mer and its reverse complement), each as a 2-bit code: first base in the highest of the 2*l bits,
 * base code (ascii >> 1) & 3 (A 0, C 1, T 2, G 3); libmdbg_emit's mdbg_lmer_filter_from_counts builds the list from the counts file with
 * the reference's rule.  n = 0 with a non-null pointer = an empty selection (no minimizer survives); codes = NULL switches the filter
 * off.  Density scheme only, l <= 32; call before the first batch (the filter is part of the sketch).  The filter applies to every
 * sketch the context computes afterwards, mdbg_query_batch included. */
int mdbg_set_lmer_filter(mdbg_ctx* ctx, const uint64_t* codes, uint64_t n);
/* Multi-k WITH contig feedback (utils/multik:69-78: every round's input is the original reads plus the previous round's contigs, twice):
 * the reads are ingested once, then mdbg_mark; per round mdbg_rewind(mark) forgets everything ingested after the mark (last round's
 * contigs) and clears the node table, mdbg_reset(k) re-windows what is resident with the round's k, and the round's contigs are
 * ingested as ordinary batches.  The reference reads the contigs BEFORE the reads (they come first in its concatenated file), and
 * DbgEntry.index / the A-th sighting follow the record order: give the reads a first_read_ordinal base above the number of contig
 * records you will ever add (e.g. 1 << 32) and the contigs the ordinals below it — only the order of the ordinals matters.
 * mdbg_rewind(mark) with the same k and no new batches restores exactly the state after the mark once mdbg_reset / mdbg_insert_resident
 * has re-inserted the resident batches.  Not valid while reserved regions are pending (MDBG_E_STATE). */
int mdbg_mark(mdbg_ctx* ctx, uint64_t* mark);
int mdbg_rewind(mdbg_ctx* ctx, uint64_t mark);

int mdbg_get_stats(mdbg_ctx* ctx, mdbg_stats* out);
/* Which HIP events the context records for the ms_* fields of mdbg_stats.  An event is a marker packet with a timestamp on the stream: about 4 microseconds of device
 * time each (scratch/ubench/event_cost.hip), i.e. ~35 microseconds per ingested batch + finalize at level 2 — 1.2 % of a 2.8-ms configs[2] step.
 *   2 (default): around the stages (ms_sketch, ms_insert, ms_finalize) and around every tile-kernel launch (ms_sketch_tile);
 *   1: around the tile-kernel launches only (ms_sketch / ms_insert / ms_finalize stay 0);   0: none (every ms_* field stays 0).
 * Results never depend on it. */
int mdbg_set_timing(mdbg_ctx* ctx, uint32_t level);
const char* mdbg_strerror(int err);
const char* mdbg_last_error(mdbg_ctx* ctx); /* detail of the last failure on ctx ("" if none) */
uint32_t mdbg_abi_version(void);
/* how the library was compiled: no bits are currently defined (bits 0 and 1 flagged experiment builds of earlier rounds), so every build returns 0. */
uint32_t mdbg_build_flags(void);
/* Device memory that contexts of this process have released is kept by the library for the next allocation (a hipMalloc that follows large
 * frees takes seconds on this stack); at most MDBG_CACHE_MB megabytes per device (environment; default a third of each device, 0 = keep nothing).
 * This hands all of it back to the runtime and returns the number of bytes released.  Never needed for the correctness of THIS library's calls: one of
 * its allocations that runs out of memory empties the cache itself before it fails.  Another allocator in the same process (torch's caching allocator,
 * RCCL, the host's own hipMalloc) does not know about the cached blocks and can run out of memory against them: such a host calls this after it has
 * destroyed its contexts (or before a large allocation of its own), or caps the cache with MDBG_CACHE_MB. */
uint64_t mdbg_release_cached_memory(void);
/* Host memory for the batches handed to mdbg_ingest_batch / mdbg_ingest_batch_packed: ordinary page-aligned memory that the first ingest call given a pointer
 * into it page-locks (hipHostRegister of the whole allocation, after the caller has written — i.e. faulted in — the batch: 0.011 ms per MB, against 0.24 ms per
 * MB for hipHostMalloc), so that the copy to the device is one DMA (57 GB/s measured) instead of the runtime's staged copy from pageable memory (17 - 20 GB/s
 * for freshly written batches).  A drop-in for malloc / free as far as the caller is concerned; memory from anywhere else is still accepted by the ingest calls
 * and takes the staged path.  mdbg_host_free keeps a
 * page-locked allocation for the next mdbg_host_alloc of about its size (unlocking and unmapping costs what locking did not: 10 ms per 73 MB), up to
 * MDBG_HOST_CACHE_MB megabytes per process (environment; default 2048, 0 = give everything back at once); mdbg_release_cached_memory releases these too.  mdbg_reader_set_allocator (mdbg_emit.h) takes this pair.  mdbg_host_is_pinned: 1 once the
 * allocation that holds p has been page-locked. */
void* mdbg_host_alloc(size_t bytes);
void mdbg_host_free(void* p);
int mdbg_host_is_pinned(const void* p);

/* ---- device-resident stage entry points (used by the multi-GPU driver and the benchmark) -------------
 * Sketch stage only, device buffers in, results appended to the context's resident sketch store. */
int mdbg_sketch_device(mdbg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n_reads,
                       uint64_t n_bases, uint64_t first_read_ordinal);
/* Window + insert every sketch appended since the last call of this function / reset. */
int mdbg_insert_resident(mdbg_ctx* ctx);
/* ---- multi-GPU: one process per GPU, reads sharded by record, ONE all-to-all of k-min-mer records ----------
 * (the exchanges themselves are done by the host driver over RCCL, see rust_mdbg_amd/dist.py)
 *
 * Key-range routing: packs every k-min-mer occurrence of the sketches not yet inserted into `world` (<= 64)
 * destination buckets, owner = mulhi64(keyhash, world).  One record is k+2 u64: canonical key, the global ordinal
 * (read ordinal << 26 | window index), the key hash.  *d_records receives a DEVICE pointer to the bucketed records
 * (library-owned, valid until the next route_pack/reset), counts[world] (HOST) the records per destination. */
int mdbg_route_pack(mdbg_ctx* ctx, uint32_t world, const uint64_t** d_records, uint64_t* counts);
/* Owner side: room for n more records at the tail of the context's arena (DEVICE pointer, valid until the next
 * arena_reserve / insert_records / reset): receive the all-to-all straight into it, then pass the same pointer to
 * mdbg_insert_records and no copy is made. */
int mdbg_arena_reserve(mdbg_ctx* ctx, uint64_t n_records, uint64_t** d_tail);
/* Owner side: insert records received from peers (DEVICE memory, k+2 u64 each).  Unless they already sit in the arena
 * tail (mdbg_arena_reserve) they are copied into it, so the caller's buffer may be released when the call returns.  After the first call the
 * context is in routed mode: mdbg_finalize is replaced by the four calls below. */
int mdbg_insert_records(mdbg_ctx* ctx, const uint64_t* d_records, uint64_t n_records);
/* Owner side: the table's entries as two query lists, each bucketed by the rank that has to answer (DEVICE pointers,
 * library-owned until the next export / finalize / reset).  Ranks are described by spans of read ordinals sorted by
 * start: span i = [span_lo[i], span_lo[i+1]) belongs to rank span_rank[i].
 *   list A, one entry per distinct k-min-mer, bucketed by the rank of its FIRST sighting: d_first[n_all] (ordinal),
 *           d_solid[n_all] (1 = passes the abundance filter, src/main.rs:922-929); counts_all[r] entries for rank r.
 *   list S, one entry per solid k-min-mer, bucketed by the rank of its A-th sighting: d_ath[n_solid] (ordinal),
 *           d_count[n_solid] (occurrences), d_slot[n_solid] (handle for mdbg_routed_keys), d_idx_all[n_solid] (position of
 *           the same k-min-mer in list A); counts_solid[r] entries for rank r. */
typedef struct mdbg_routed_lists {
    uint64_t n_all, n_solid;
    const uint64_t* d_first; const uint8_t* d_solid;
    const uint64_t* d_ath; const uint32_t* d_count; const uint64_t* d_slot; const uint64_t* d_idx_all;
    uint64_t counts_all[64], counts_solid[64];
} mdbg_routed_lists;
int mdbg_routed_export(mdbg_ctx* ctx, uint32_t world, const uint64_t* span_lo, const uint32_t* span_rank, uint32_t n_spans,
                       mdbg_routed_lists* out);
/* Generator side (the rank whose reads the ordinals belong to): for n first-sighting ordinals (DEVICE) with their solid
 * flags, rank_first[i] = number of queried ordinals smaller than ord[i] (-> DbgEntry.index once the totals of the ranks
 * holding earlier reads are added), rank_solid[i] = the same among solid ones (-> row of the node in index order).
 * ALL queries for this rank must be passed in one call.  Outputs are caller-owned DEVICE buffers of n u64. */
int mdbg_resolve_first(mdbg_ctx* ctx, const uint64_t* d_ord, const uint8_t* d_solid, uint64_t n, uint64_t* d_rank_first,
                       uint64_t* d_rank_solid, uint64_t* total_first, uint64_t* total_solid);
/* Generator side: what the reference stores from the sighting with ordinal ord[i] (src/main.rs:675-684,778), 6 u64 per
 * query into the caller-owned DEVICE buffer d_meta: {seqlen | reversed << 32, shift0, shift1, src_read, src_start,
 * src_end}; all zero for ord[i] == ~0. */
int mdbg_resolve_meta(mdbg_ctx* ctx, const uint64_t* d_ord, uint64_t n, uint64_t* d_meta);
/* Owner side: canonical keys (k u64 each) of the given slot handles into the caller-owned DEVICE buffer d_keys. */
int mdbg_routed_keys(mdbg_ctx* ctx, const uint64_t* d_slot, uint64_t n, uint64_t* d_keys);
/* ---- graph edges (replaces the single-threaded edge loop of src/main.rs:1017-1117) ------------------------------
 * Edges of the node table produced by the LAST mdbg_finalize / mdbg_finalize_device on this context (the table stays on
 * the device): for every node n1 and both of its (k-1)-mers, the nodes listing the same normalized (k-1)-mer, the four
 * orientation tests (main.rs:1062-1075), abundance presimplification (main.rs:1078-1090 and 1104-1115; presimp = 0
 * disables it, the reference's default is 0.01) and overlap = min(n1.seqlen - shift(ori1), n2.seqlen - 1).  n1/n2 are
 * DbgEntry.index values, o1/o2 are '+' / '-'.  The order is the one a sequential pass over the node table produces
 * (n1 in table order, suffix key before prefix key, listings in table order, orientations ++, +-, -+, --); the
 * reference iterates a DashMap, so only the multiset of its L lines is defined.
 * mdbg_graph_edges: HOST arrays owned by the context; mdbg_graph_edges_device: DEVICE arrays; both valid until the next
 * edge call.  The layout equals mdbg_edges of include/mdbg_emit.h, so the host copy can go straight to mdbg_emit_write_gfa. */
typedef struct mdbg_edge_list {
    uint64_t n;
    const uint32_t* n1; const uint8_t* o1; const uint32_t* n2; const uint8_t* o2; const uint32_t* overlap;
    uint64_t presimp_removed;     /* candidate edges dropped by the abundance rule (before the symmetric removal) */
} mdbg_edge_list;
int mdbg_graph_edges(mdbg_ctx* ctx, float presimp, mdbg_edge_list* out);
int mdbg_graph_edges_device(mdbg_ctx* ctx, float presimp, mdbg_edge_list* out);

/* ---- unitigs and the base-space copy plan (replaces `gfatools asm -u` + the planning half of src/to_basespace.rs) --------
 * Every documented run of the reference pipes its .gfa through `gfatools asm -u` (compaction of non-branching paths) and the
 * to_basespace binary to get sequences; this is that step — and only that step: no tip or bubble removal (magic_simplify's
 * -t / -b rounds: see mdbg_graph_simplify below) — on the node table of the last mdbg_finalize* and the edge list of the last mdbg_graph_edges* of the context
 * (with whatever presimp that call used).  MDBG_E_STATE without a current edge list (a finalize or an ingest since the last edge
 * call), and on routed / partitioned contexts: SINGLE-GPU ONLY.  An empty context gives an empty list.
 *
 * Definition (gfatools' own names and orientation choices are not reproduced):
 *   vertex = (node, orientation), comp(v) flips the orientation.  Arcs = the DISTINCT (n1,o1)->(n2,o2) of the edge records together
 *   with their mirrors (n2,!o2)->(n1,!o1).  u->v is a LINK iff u has exactly one distinct out-arc, v exactly one distinct in-arc and
 *   node(u) != node(v); chains of links come in disjoint mirror pairs, and a unitig is one maximal chain of each pair:
 *     linear    the orientation whose first node has the smaller index (a single node: '+');
 *     circular  the orientation that holds the cycle's smallest-index node as '+', starting at that node.
 *   Unitigs are ordered by the index of their first node; unitig i is named "utg%07d" (i + 1) followed by 'l' or 'c'
 *   (to_basespace.rs:89,103,294).
 *   edges: every edge record whose arc is not an interior link, in source order, duplicates kept, as (unitig, +/-, unitig, +/-,
 *   overlap) with n1 / n2 = 0-based unitig numbers; the closing link of a circular unitig u gives "u + u +" (its mirror "u - u -").
 *   An overlap larger than either unitig's length becomes min(len_src - 1, len_sink - 1) (to_basespace.rs:312-320).
 *   Walk of unitig i = entries offsets[i] .. offsets[i+1]: node[] (DbgEntry.index), ori[] ('+' / '-'), and the piece of the unitig's
 *   sequence the entry contributes (to_basespace.rs:132-153,203-262, with seq = the node's .sequences sequence and (s0, s1) its
 *   shift_full: first entry '+' all of seq, '-' revcomp(seq); later entries '+' the last s1 bases of seq, '-' revcomp of the first s0
 *   bases), stored in READ coordinates: bases [src_begin, src_begin + len) of read src_read go to [dst_offset, dst_offset + len) of
 *   the unitig, passed through utils::revcomp `revcomp` times (0: copied; 1: reverse-complemented; 2: in read order, but through
 *   revcomp's byte map twice — a node whose sequence is itself a reverse complement, walked '-').  dst_offset is the running sum of
 *   len inside the unitig and length[] (the LN tag) its total; kc_sum[] the sum of the nodes' abundances (the writer prints
 *   mc:f = kc_sum / entries, to_basespace.rs:265-288); circular[] 0 / 1.  mdbg_emit_contigs_* (mdbg_emit.h) executes the plan.
 * mdbg_graph_unitigs: HOST arrays; mdbg_graph_unitigs_device: DEVICE arrays; owned by the context until its next unitig, simplify, edge,
 * finalize or reset call (mdbg_graph_contigs reads the device arrays of the last call whichever variant was used).  n_rounds: pointer-jumping rounds the call ran (at most ceil(log2(2 n)) + 1 to rank the paths, as many
 * again where there are cycles; a ranking that does not settle inside the bound is reported as MDBG_E_DEVICE, never looped on). */
typedef struct mdbg_unitig_list {
    uint64_t n_unitigs, n_entries;
    const uint64_t* offsets;      /* n_unitigs + 1 */
    const uint32_t* node; const uint8_t* ori;                                             /* n_entries: the walk */
    const uint64_t* src_read; const uint64_t* src_begin; const uint32_t* len; const uint8_t* revcomp; const uint64_t* dst_offset;  /* n_entries: the copy plan */
    const uint64_t* length; const uint64_t* kc_sum; const uint8_t* circular;              /* n_unitigs */
    mdbg_edge_list edges;         /* unitig edges; presimp_removed = 0 */
    uint32_t n_rounds, reserved;
} mdbg_unitig_list;
int mdbg_graph_unitigs(mdbg_ctx* ctx, mdbg_unitig_list* out);
int mdbg_graph_unitigs_device(mdbg_ctx* ctx, mdbg_unitig_list* out);

/* ---- graph simplification: tip clipping, simple-bubble popping (the -t / -b rounds of utils/magic_simplify), small-component removal and
 * ---- the pruning of edges no read crosses ----
 * Runs a caller-given schedule of steps on the GPU and returns the unitig list (same layout, same ownership rule, same state
 * requirements as mdbg_graph_unitigs: a current edge list, SINGLE GPU ONLY) of the graph that is left.  With n_steps = 0 the result
 * equals mdbg_graph_unitigs array for array.  The first `gfatools asm` line of utils/magic_simplify is the schedule
 * t t b b t b b b t b t B T B with t = {TIPS, 10, 50000}, b = {BUBBLES, 0, 100000}, B = {BUBBLES, 0, 1000000}, T = {TIPS, 10, 150000}.
 *
 * THE RULES ARE THIS PROJECT'S OWN DEFINITION, NOT BIT-PARITY WITH GFATOOLS.  gfatools deletes in place while it scans, so its result
 * depends on vertex order; the rules below are order-free (a parallel implementation and a dictionary-and-set checker must agree:
 * tests/simplify_restatement.py).  The two outputs have never been compared.
 *
 *   State: a set S of surviving nodes, at first all nodes of the table, and a set D of removed arcs, closed under mirroring and at first
 *   empty.  The current graph is the arc set of mdbg_graph_unitigs restricted to arcs whose two nodes are in S, minus D; the current
 *   unitigs are its unitigs by the definition above (order, orientation, names, length, kc_sum unchanged).  Every step kind decides on
 *   that graph, as it is when the step starts, and every compaction compacts it.  A TIPS, BUBBLES or COMPONENTS step chooses unitigs
 *   to remove and removes all their nodes from S; an EDGES step chooses edge records and puts their arcs into D.
 *   A unitig is SMALL for a step iff it is not circular, has at most max_nodes entries and length <= max_bases (0 = no limit).
 *   a BEATS b: higher mean abundance kc_sum / entries (compared exactly by cross-multiplication), then larger length, then the
 *   smaller unitig number.
 *   TIPS.  Orient a small unitig u so that its first vertex has no in-arc.  u is a tip candidate iff that is possible in exactly
 *   one of its two orientations (a unitig with two dead ends is an isolated piece and is never removed by this kind: a deliberate
 *   difference from gfatools; COMPONENTS below removes such pieces); x = the last vertex in that orientation, its attached vertex.  u is removed iff for every arc x -> w the vertex w has
 *   another in-neighbour x' != x that is not the attached vertex of a tip candidate, or is the attached vertex of a candidate that
 *   beats u.  Hence a vertex that survives and had an in-arc keeps one: clipping never makes a new dead end, and where every way
 *   into w is a small tip the best one stays.
 *   BUBBLES (simple ones only).  A small unitig u with first vertex f and last vertex t is a branch iff f has exactly one in-arc
 *   p -> f, t exactly one out-arc t -> q, neither node(p) nor node(q) lies on u, and q != comp(p).  Its key is the smaller of (p, q)
 *   and (comp(q), comp(p)) under the vertex order 2 * index + minus.  Of the branches with one key all but the one that beats the
 *   others are removed.  Branches that branch themselves are not treated by this kind (repeated tip and bubble steps reduce many
 *   of them to simple ones); they are the SUPERBUBBLES kind's, below.
 *   COMPONENTS.  The step decides against the current unitigs and their edges as they are when the step starts, grouped into connected components
 *   by the definition of mdbg_graph_components below.  A component is SMALL for the step iff its `circular` is 0, its `nodes` <= max_nodes and its
 *   `bases` <= max_bases (0 = no limit on that side): the limits apply to the component's sums, not to one unitig.  Every unitig of a small component
 *   is removed; unitigs_removed[k] / nodes_removed[k] count as for the other kinds.  max_nodes == 0 && max_bases == 0 is MDBG_E_PARAM for this kind
 *   (it would delete the graph).  A step may remove everything that is left: the call then returns MDBG_OK with the empty list (n_unitigs ==
 *   n_entries == 0, edges.n == 0).  The schedule of utils/magic_simplify has no such step.
 *   EDGES, {MDBG_SIMPLIFY_EDGES, min_support, 0}: for this kind the field max_nodes carries min_support (>= 1) and max_bases is reserved (0).  An edge of
 *   the graph does not come from a read (mdbg_graph_junctions below): a repeat of exactly k-1 minimizers that two contexts share puts a full 2 x 2 cross of
 *   edges into the graph, two of which no read ever took.  The step decides against the edge records of the current unitig list as they are when the
 *   step starts.  support[r] is what mdbg_graph_junctions gives for record r of that list over the WHOLE resident store (first_read = 0, max_reads = 0).
 *   Let x -> y be the node-level arc of r: x the last vertex of n1 in orientation o1, y the first vertex of n2 in orientation o2.  r is STRONG iff
 *   support[r] >= min_support, else WEAK.  A vertex v HAS A STRONG EXIT iff some strong record has an arc, or the mirror of its arc, with source v.  A weak
 *   record is REMOVED iff x has a strong exit and comp(y) has a strong exit — reads leave x another way, and reads enter y another way; its arc and the
 *   mirror arc join D.  Records with equal junction keys carry equal supports, so a record, its mirror record and their duplicates fall together.
 *   Consequences: an interior link is never removed (it is the only exit of its source, and it has no record); a weak edge that is the only way, supported
 *   or not, out of a dead-end side stays, so a coverage gap does not cut a contig; the step removes no node (unitigs_removed[k] == nodes_removed[k] == 0
 *   for it); a compaction follows iff it removed a record; if no read is resident nothing is strong and the step removes nothing.  The removed records are
 *   counted by mdbg_simplify_edges_removed.
 *   REPEATS, {MDBG_SIMPLIFY_REPEATS, min_support, 0}: as for EDGES, max_nodes carries min_support (>= 1) and max_bases is reserved (0).  The step duplicates the
 *   unitigs the resident reads resolve (mdbg_graph_transits below), so that the next compaction makes contigs that cross the repeat.  It decides against the
 *   current unitig list L as it is when the step starts, with what mdbg_graph_transits gives for L over the WHOLE resident store (first_read = 0, max_reads = 0) at
 *   that min_support.  Vertex (u, j, s), pair, mirror, key, link and m(u) are those of the junction and transit definitions.  A unitig u is RESOLVED iff
 *   verdict[u] == MDBG_TRANSIT_RESOLVED; its strong keys, in key order, are (u, p_0, q_0) < ... < (u, p_{m-1}, q_{m-1}) with m = n_in[u] = n_out[u] >= 2, and by the
 *   verdict the p are pairwise different and so are the q.
 *   Copies.  Let X = 1 + the largest DbgEntry.index of the node table.  Go through the resolved unitigs in ascending u, for each through i = 1 .. m-1, and within
 *   that through the entries j = 0 .. m(u)-1 of u's walk: the copy (u, i, j) is a new node with index X + c, c counting from 0 in that order.  A copy has every
 *   column of its original (abundance, source read and span, shift, reversed); copy i = 0 is the originals themselves.  Abundances are not divided: kc_sum counts
 *   the repeat's windows in every copy.
 *   Arcs.  Take every edge record of the current graph (both nodes in S, its arc not in D); its pair is (x, y) in L's coordinates.  An interior link of a resolved
 *   u stays, and for every i >= 1 one more record joins the copies (u, i, .) of its two nodes, with the same orientations and the same overlap.  Otherwise each of
 *   its two ends is treated on its own.  Source end: if x == (u, m(u)-1, 0) with u resolved, the end belongs to the i with q_i == y; if x == (u, 0, 1), to the i
 *   with p_i == (y.u, y.j, 1 - y.s).  Target end: if y == (u, 0, 0), to the i with p_i == x; if y == (u, m(u)-1, 1), to the i with q_i == (x.u, x.j, 1 - x.s).  The
 *   node at that end is replaced by its copy i (i = 0: unchanged).  Exactly one such i exists, because the matching is perfect and n_in == m; if the device finds
 *   none or two, that is a defect: MDBG_E_DEVICE, nothing guessed and nothing indexed outside.  A record that joins two resolved unitigs is redirected at both ends.
 *   Consequences: a record, its mirror record and their duplicates move together (equal junction keys); no record is removed; every copy of u has exactly one
 *   distinct in-arc and one distinct out-arc; the step removes nothing (unitigs_removed[k] == nodes_removed[k] == 0, and its mdbg_simplify_edges_removed entry is
 *   0); a compaction follows iff the step copied something; with no resident reads nothing resolves.
 *   State afterwards: S gains the copies and the arc set is the redirected one.  TIPS, BUBBLES and COMPONENTS steps behind it run unchanged on that graph, and
 *   their nodes_removed count copies like nodes.  Unitig order and orientation ("index of the first node") use the copies' indices; the list's node[] reports the
 *   ORIGINAL's index, so an index may occur in several entries.  n_entries == rows of the node table - total_nodes_removed + copies.
 *   Limits of this round, MDBG_E_PARAM while the schedule is validated: min_support == 0, max_bases != 0, more than one REPEATS step in a schedule, an EDGES step
 *   behind a REPEATS step (reads cannot be placed on copied nodes).  MDBG_E_CAPACITY: 2^30 rows including the copies, or 2^32 records including the added ones.
 *   A list that holds copies: mdbg_graph_read_paths*, mdbg_graph_junctions* and mdbg_graph_transits* on it answer MDBG_E_STATE (a table row would belong to several
 *   entries); the context stays usable, and a list built by a REPEATS step that copied nothing is placed as always.  mdbg_graph_components*, mdbg_graph_contigs* and
 *   the emitters work on it unchanged: they read the list, not the table.  Placing reads on copies, and with it a second round of resolution, is the NESTED
 *   kind's (below); the REPEATS kind keeps meaning "the graph holds no copies", and everything said here about it stays as it is.
 *   The number of copied entries follows from the identity above (a schedule holds at most one such step); a per-step count of resolved unitigs would need a new
 *   entry point and waits for a change that may touch the number of prototypes.
 *   NESTED, {MDBG_SIMPLIFY_NESTED, min_support, 0}: a repeats step that may stand anywhere in a schedule, in particular behind a REPEATS step or another NESTED
 *   step, any number of times: a repeat whose middle occurs elsewhere too becomes one unitig only when its middle has been resolved, and the next step resolves it.
 *   max_nodes carries min_support (>= 1) and max_bases is reserved (0).  The step decides against the current list L as it is when the step starts, copies included,
 *   with the transits of L over the whole resident store under the placement on a list that holds copies (below).  Verdicts, strong keys, copies, arcs and
 *   consequences are the REPEATS text, with these additions.
 *   Originals.  origin(x) of a node is the DbgEntry.index of the table row it descends from: an original is its own origin, the origin of a copy of a copy is the
 *   table row's.  A copy has every column of the node it was copied from.
 *   Indices.  X stays 1 + the largest DbgEntry.index of the node table for the whole schedule; the copies of a later step continue the numbering behind all earlier
 *   copies of the schedule, in the same order (ascending u, then i, then j).
 *   Reported list.  At the end of the schedule node[] reports the origin.  n_entries == rows of the node table - total_nodes_removed + all copies of the schedule.
 *   No copies yet.  On a graph that holds no copies the step IS the REPEATS step: the same launches, the same waits, the same arrays.
 *   MDBG_E_PARAM while the schedule is validated: min_support == 0, max_bases != 0, an EDGES step behind a NESTED step (edge pruning on a graph that holds copies is
 *   not in this change), a REPEATS step behind a NESTED step.  MDBG_E_CAPACITY and the defect flags are those of REPEATS.  After a schedule whose NESTED step copied
 *   something mdbg_graph_read_paths*, mdbg_graph_junctions* and mdbg_graph_transits* go on answering MDBG_E_STATE, as after REPEATS.
 *   PLACEMENT ON A LIST THAT HOLDS COPIES.  row(e) of list entry e is the table row of origin(node of e).  mult(r) is the number of entries e of L with row(e) == r;
 *   removed nodes are not entries, so a copy that a TIPS step removed makes its row unique again.  A window whose key is row r of the node table (the test of
 *   mdbg_graph_read_paths) is: not placed if mult(r) == 0; UNIQUE if mult(r) == 1, placed on that entry as always; AMBIGUOUS if mult(r) >= 2.  Windows are numbered
 *   along their read.  For an AMBIGUOUS window w the LEFT ANCHOR is the nearest window a < w of the same read that is not AMBIGUOUS, provided it is UNIQUE: if that
 *   window is not placed, or the read starts first, w has no left anchor.  With the anchor on entry e_a in strand s_a the LEFT CANDIDATE is the entry
 *   e = e_a + (w - a) if s_a == 0, e_a - (w - a) if s_a == 1.  It is VALID iff e lies in the same unitig as e_a (no wrap, also on a circular unitig), row(e) is w's
 *   row, and rev(w) XOR (ori[e] == '-') == s_a.  The RIGHT ANCHOR b > w and the RIGHT CANDIDATE are defined alike: e_b - (b - w) if s_b == 0, e_b + (b - w) if
 *   s_b == 1.  Verdict on w: both candidates valid and equal, or exactly one valid: w is placed there, in the anchor's strand; both valid and different (a CONFLICT)
 *   or none valid: w is not placed.  Links, crossings, explained crossings, transits and the consequence "a transit walks all of one unitig" are the existing text
 *   over these placements.  Every window decides alone from its own two anchors, so the result is order-free and two calls give identical arrays.
 *   Waits.  A NESTED step on a graph with copies waits as a REPEATS step does: once for its transit stage (the placement's extra launches — one kernel, two scans,
 *   one kernel — ride in it) and, if something resolves, twice more; the one wait at the end of the schedule maps node[] to the origins of all copies.
 *   The placement counts its ambiguous windows and those it placed (resolved), found in conflict, or left without a valid candidate (unanchored).  The ABI has no
 *   room for them: with MDBG_NESTED_STATS in the environment a simplify call with a NESTED step writes them, summed over its NESTED steps on a graph with
 *   copies, as one line to stderr.  That line is a diagnostic for measurements and tests, NOT part of this interface: its name and form may change or go without
 *   a new ABI version, and no program should depend on it.
 *   SUPERBUBBLES, {MDBG_SIMPLIFY_SUPERBUBBLES, max_nodes, max_bases}: what `gfatools asm -b` (gfa_pop_bubble) is after — a bubble whose inside branches again, is
 *   cross-linked or holds bubbles of its own — by an order-free rule.  Like every kind the step decides against the graph as it is when the step starts.  Vertices:
 *   the oriented current unitigs (u, strand).  Arcs: the unitig edge records between surviving nodes whose arc is not in D, plus their mirrors; parallel records
 *   and duplicates count as one arc.  For a vertex s with at least two distinct out-neighbours, (s, t) BOUNDS A SUPERBUBBLE WITH INTERIOR I iff I is a non-empty
 *   set of vertices, s and t are not in I, t != s, and
 *     (a) every out-neighbour of s and of every x in I lies in I + {t}, and every x in I has at least one (an interior dead end is the TIPS step's business);
 *     (b) every in-neighbour of t and of every x in I lies in I + {s}, and every x in I has at least one (the mirror image of (a): with it the mirror reading
 *         below is a superbubble by the same text, and I is exactly what s reaches without leaving t);
 *     (c) the arcs among I + {s, t} contain no cycle;
 *     (d) no two members of I + {s, t} are each other's complement, so the unitigs involved are pairwise different (hence no circular unitig is inside);
 *     (e) t is the first such vertex: no t' in I bounds a superbubble with s over a subset of I;
 *     (f) |I| <= MDBG_SUPERBUBBLE_MAX_UNITIGS.
 *   The bubble FITS iff max_nodes == 0 or the entries of the unitigs of I sum to at most max_nodes, and max_bases == 0 or their `length` sums to at most
 *   max_bases (overlaps are counted twice: a limit, not a measure).  Both 0 is allowed; (f) still bounds it.
 *   (s, t, I) and its mirror (comp t, comp s, comp I) are one bubble; the reading whose source has the smaller (unitig number, strand) is the CANONICAL one, and it
 *   alone decides which path is kept.
 *   Kept path.  mean(x) = kc_sum / entries, compared exactly by cross products.  val(s) = +infinity; for x in I in any topological order best(x) is the in-neighbour
 *   with the largest val, ties going to the one that BEATS the other (the total order above: mean, then length, then the smaller number), and
 *   val(x) = min(mean(x), val(best(x))); best(t) is chosen likewise.  The kept path is t, best(t), best(best(t)), ... back to s: the path whose weakest unitig is
 *   strongest.  When every branch is a single unitig this is the BUBBLES rule's winner.
 *   Applied bubbles.  Let J be the union of I + comp(I) over all fitting bubbles.  A fitting bubble is APPLIED iff neither s nor comp(t) lies in J: the outermost
 *   fitting bubble wins, an inner one pops only when the bubble around it does not fit or is no bubble, and back-to-back bubbles that share t = s' are both applied.
 *   Removal.  Every unitig of an applied bubble's I that is not on its kept path is removed; unitigs_removed[k] / nodes_removed[k] count as for TIPS.  The step
 *   removes no record of its own and never removes s or t; a compaction follows iff something was removed; behind a REPEATS step it runs unchanged on the larger
 *   graph, and behind an EDGES step it sees the masked arcs.  Two fitting bubbles are nested or have disjoint interiors, so applied bubbles never touch each
 *   other's kept path (tests/superbubble_restatement.py asserts it on every graph it sees).
 *   Result: n_entries = |S|; edges = every edge record whose two nodes survive, whose arc is not in D and is not an interior link, in source order.
 * An EDGES step needs what mdbg_graph_junctions needs on top of a current edge list — the node table current, the bounds of the read paths —, and the call
 * refuses with the same code before anything is launched; the context stays usable.  The step uses the context's junction buffers: a junction result the
 * caller holds ends with a simplify call that has an EDGES step, exactly as a component result ends with one that has a COMPONENTS step; a held read-path,
 * component or contig result is untouched.  The defect flags of the junction stage surface as MDBG_E_DEVICE.
 * A REPEATS step needs what mdbg_graph_transits needs, and the call refuses with the same codes before anything is launched.  It uses the context's transit
 * buffers and placement scratch: a transit result the caller holds ends with a simplify call that has a REPEATS step; after such a call mdbg_transits_ms gives the
 * device time of the step's transit stage.  It waits once for its transit stage and, if something resolves, twice more (the totals that size the copies, its
 * defect flag); one more wait at the end of the schedule maps node[] to the originals.
 * A NESTED step needs and uses what a REPEATS step does.
 * MDBG_E_PARAM: an unknown kind, a COMPONENTS step without a limit, an EDGES, REPEATS or NESTED step with min_support == 0 or max_bases != 0, a second REPEATS step, an EDGES step behind a REPEATS or NESTED step, a REPEATS step behind a NESTED step, steps == NULL with n_steps > 0, stats == NULL.  stats->unitigs_removed / nodes_removed: n_steps HOST
 * entries owned by the context (valid like the list); n_compactions: compactions run (a step that removes nothing is followed by none);
 * n_syncs: host synchronisations of the call (per step: those of one compaction + 1; a COMPONENTS step adds none of its own; an EDGES step that has
 * records and resident reads to look at waits twice — the one wait of its junction stage, then its own counter, which the junction stage's wait cannot
 * carry because the decision reads the supports — and is followed by a compaction only if it removed a record).
 * mdbg_simplify_edges_removed: *per_step <- n_steps HOST entries of the last simplify call, owned by the context and valid like unitigs_removed;
 * per_step[k] = the node-level edge records step k put into D (mirror records and duplicates counted as records; 0 for the other kinds); *total <- their
 * sum.  Either pointer may be NULL.  mdbg_simplify_stats keeps its layout. */
#define MDBG_SIMPLIFY_TIPS 1u
#define MDBG_SIMPLIFY_BUBBLES 2u
#define MDBG_SIMPLIFY_COMPONENTS 4u
#define MDBG_SIMPLIFY_EDGES 8u     /* {EDGES, min_support, 0} */
#define MDBG_SIMPLIFY_REPEATS 16u  /* {REPEATS, min_support, 0} */
#define MDBG_SIMPLIFY_SUPERBUBBLES 64u   /* {SUPERBUBBLES, max_nodes, max_bases}; 32 is no kind */
#define MDBG_SIMPLIFY_NESTED 128u  /* {NESTED, min_support, 0} */
#define MDBG_SUPERBUBBLE_MAX_UNITIGS 64u /* (f): the interior and the sink of one bubble fit the 2 x 64 slots of one wave */
typedef struct mdbg_simplify_step { uint32_t kind, max_nodes; uint64_t max_bases; } mdbg_simplify_step;
typedef struct mdbg_simplify_stats {
    uint32_t n_steps, n_compactions;
    const uint64_t* unitigs_removed; const uint64_t* nodes_removed;      /* n_steps */
    uint64_t total_unitigs_removed, total_nodes_removed;
    uint32_t n_rounds_total, n_syncs;
} mdbg_simplify_stats;
int mdbg_graph_simplify(mdbg_ctx* ctx, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats);
int mdbg_graph_simplify_device(mdbg_ctx* ctx, const mdbg_simplify_step* steps, uint32_t n_steps, mdbg_unitig_list* out, mdbg_simplify_stats* stats);
int mdbg_simplify_edges_removed(mdbg_ctx* ctx, const uint64_t** per_step, uint64_t* total);

/* ---- connected components of the unitig graph ---------------------------------------------------------------------------------
 * Which unitigs belong together: what the reference's users get from splitting a .gfa by weakly connected component.  The call works on the context's
 * CURRENT unitig list — the device arrays left by the last mdbg_graph_unitigs* / mdbg_graph_simplify* call, the list mdbg_graph_contigs uses — and leaves the
 * node table, the edge list and the unitig list untouched (a contig call after it gives the same bytes).  SINGLE GPU ONLY.
 *
 * Definition:
 *   Two unitigs of the list are JOINED iff some record of the list's `edges` names both of them, one as n1 and the other as n2; orientation is ignored,
 *   and a record with n1 == n2 joins nothing.  A COMPONENT is a class of the transitive closure of "joined"; a unitig with no edge to another unitig is a
 *   component of its own.  Components are numbered 0, 1, ... by the number of their smallest unitig.  Per component:
 *     first_unitig  its smallest unitig number;                      unitigs   how many unitigs it holds;
 *     nodes         the sum of offsets[u+1] - offsets[u] over them;   bases     the sum of length[u];
 *     kc_sum        the sum of kc_sum[u];                             circular  1 iff any member unitig is circular.
 *   Everything is an integer sum or a minimum: the result does not depend on scheduling, and two calls give identical arrays.
 * mdbg_graph_components: HOST arrays; mdbg_graph_components_device: DEVICE arrays.  They belong to the context until its next component call, its next
 * simplify call with a COMPONENTS step, or a call that ends the unitig list; they share no buffer with the unitig list, the contig result or the
 * node-sequence result.  The device variant waits for the device ONCE (the component count and the defect flag in one read-back); the number of kernel launches
 * is fixed.  The union-find behind it bounds every loop by n_unitigs + 1 steps; running into the bound is reported as MDBG_E_DEVICE, never waited on.
 * MDBG_E_STATE: no current unitig list, or a routed / partitioned context; MDBG_E_PARAM: a null pointer.  An empty list gives MDBG_OK with zero counts. */
typedef struct mdbg_component_list {
    uint64_t n_unitigs, n_components;
    const uint32_t* component;                         /* n_unitigs: component number of unitig u */
    const uint32_t* first_unitig; const uint32_t* unitigs;      /* n_components */
    const uint64_t* nodes; const uint64_t* bases; const uint64_t* kc_sum; const uint8_t* circular;   /* n_components */
} mdbg_component_list;
int mdbg_graph_components(mdbg_ctx* ctx, mdbg_component_list* out);
int mdbg_graph_components_device(mdbg_ctx* ctx, mdbg_component_list* out);

/* ---- contigs stitched on the GPU from reads kept packed in device memory -----------------------------------------------------
 * A context created with MDBG_FLAG_KEEP_READS in mdbg_params.flags keeps, for every batch that goes through an entry point WITH bases (mdbg_ingest_batch, _device,
 * _packed, _packed_device, mdbg_sketch_device, mdbg_sketch_packed_device), a device copy in the layout of mdbg_packed_batch: the two 32-bit planes per 32 bases,
 * the read offsets and the exception side-list (position, original byte), so the copy is lossless.  ASCII batches are packed on the device (the kernel behind
 * mdbg_pack_device; the side-list is sorted on the device too), packed batches are copied device to device.  The store lives as the sketch store does:
 * mdbg_reset(ctx, 0) drops everything, mdbg_reset(ctx, k != 0) keeps everything, mdbg_rewind(mark) drops exactly the batches ingested after the mark.
 * Batches without bases (mdbg_ingest_sketch, mdbg_sketch_commit*, routed records) cannot be kept; they stay legal, and mdbg_graph_contigs then answers
 * MDBG_E_STATE.  SINGLE GPU ONLY, like the unitig stage.  Without the flag the ingest path is what it was: no allocation, no launch, no branch in a kernel.
 * mdbg_kept_reads: what the store holds now; *bytes = the bytes of its arrays: per batch 8 * ceil(bases / 32) + 8 * (reads + 1) + 9 * exceptions, i.e.
 * bases / 4 + 8 per read + 9 per exception up to the rounding of each batch (the device blocks that hold them may be larger: the library's block cache hands out
 * blocks of up to twice the size asked for).  Any of the three pointers may be NULL.
 *
 * mdbg_graph_contigs executes the copy plan of the context's CURRENT unitig list — the device arrays left by the last mdbg_graph_unitigs* / mdbg_graph_simplify*
 * call; a later edge, finalize, ingest, rewind or reset call ends it — against the kept reads, byte for byte as mdbg_emit_contigs_add_batch (mdbg_emit.h) does
 * on the host: revcomp 0 copies, 1 reverse-complements through utils::revcomp's byte map (N and every byte outside ACGTUacgtu become N), 2 maps every byte through
 * that map twice in read order.  Only unitigs with length >= min_len are produced, in list order (`seqtk seq -L`); unitig[i] = the 0-based number of contig i in
 * the unitig list.  With min_len = 0 every unitig is produced and offsets[] is the running sum of length[].
 * MDBG_E_STATE: no current list, a context without the flag, a routed / partitioned context, or a plan entry whose read is not kept; MDBG_E_PARAM: a plan entry
 * outside its read (reported through a flag the kernel sets; nothing is read out of bounds).
 * mdbg_graph_contigs: HOST arrays; mdbg_graph_contigs_device: DEVICE arrays (bases 16-byte aligned).  Both belong to the context until its NEXT CONTIG CALL or
 * mdbg_destroy, and to nothing else: they survive mdbg_rewind, mdbg_reset and ingest calls, so a round's contigs can be ingested (mdbg_ingest_batch_device with
 * bases / offsets / n_contigs / n_bases) as the next round's input without leaving the device.
 * mdbg_contigs_ms: device time of the stitch kernel of the last contig call (HIP events; 0 if it produced no bases). */
typedef struct mdbg_contig_seqs {
    uint64_t n_contigs, n_bases;
    const uint8_t*  bases;     /* n_bases ASCII bytes, contig after contig */
    const uint64_t* offsets;   /* n_contigs + 1 */
    const uint64_t* unitig;    /* n_contigs: 0-based number of the contig in the unitig list it was built from */
} mdbg_contig_seqs;
int mdbg_graph_contigs(mdbg_ctx* ctx, uint64_t min_len, mdbg_contig_seqs* out);
int mdbg_graph_contigs_device(mdbg_ctx* ctx, uint64_t min_len, mdbg_contig_seqs* out);
int mdbg_kept_reads(mdbg_ctx* ctx, uint64_t* n_reads, uint64_t* n_bases, uint64_t* bytes);
int mdbg_contigs_ms(mdbg_ctx* ctx, double* ms);

/* ---- node sequences gathered on the GPU from the kept reads: what the .sequences writer needs, without a second pass over the input ------------
 * The sequence of row i of the context's CURRENT node table (the table of the last mdbg_finalize* call, in index order; a table of mdbg_finalize_gfa is fine, the
 * device rows are all there) is bytes [src_start[i], src_end[i]) of read src_read[i], copied as they are if reversed[i] == 0 and otherwise through utils::revcomp
 * (src/utils.rs:3-24: reversed, N and every byte outside ACGTUacgtu become N) — byte for byte what mdbg_seqfile_write_batch (mdbg_emit.h) prints in a row's line.
 * The rows of a table overlap heavily (consecutive nodes share k - 1 minimizers), so together they are many times the input: a call hands out a CHUNK, rows
 * [first_row, first_row + n_rows) with n_rows the largest count <= max_rows whose sequences together are <= max_bases bytes.  At least one row is produced while
 * first_row < n, so a row longer than the budget comes alone; max_rows = 0 / max_bases = 0: no limit on that side; first_row >= n: MDBG_OK with n_rows = 0,
 * which ends a caller's loop `first_row += n_rows`.  mdbg_seqfile_write_nodes (mdbg_emit.h) takes a chunk as it is.
 * mdbg_graph_node_seqs: HOST arrays; mdbg_graph_node_seqs_device: DEVICE arrays (bases 16-byte aligned).  Both belong to the context until its NEXT
 * NODE-SEQUENCE CALL or mdbg_destroy; they share no memory with the contig result, so a caller may hold a mdbg_graph_contigs result and a chunk at once.
 * The calls leave the node table, the edge list and the unitig list as they are.  The rows' lengths are summed once per node table, not once per chunk; a call
 * waits for the device twice at most (the chunk's size, the error flag).
 * MDBG_E_STATE: a context without MDBG_FLAG_KEEP_READS, a routed / partitioned context (SINGLE GPU ONLY), no current node table (an ingest, rewind or reset call
 * that followed the finalize ended it), or a resident batch that came without bases; MDBG_E_PARAM: a row outside its read (reported through a flag the kernel
 * sets; nothing is read out of bounds).  The finalize of a context with nothing resident leaves a table of no rows: MDBG_OK, n_rows = 0.
 * mdbg_node_seqs_ms: device time of the gather kernel of the last node-sequence call (HIP events; 0 if it produced no bases). */
typedef struct mdbg_node_seqs {
    uint64_t first_row, n_rows, n_bases;
    const uint8_t*  bases;     /* n_bases ASCII bytes, row after row, each already oriented as its .sequences line prints it */
    const uint64_t* offsets;   /* n_rows + 1, offsets[0] = 0 */
} mdbg_node_seqs;
int mdbg_graph_node_seqs(mdbg_ctx* ctx, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out);
int mdbg_graph_node_seqs_device(mdbg_ctx* ctx, uint64_t first_row, uint64_t max_rows, uint64_t max_bases, mdbg_node_seqs* out);
int mdbg_node_seqs_ms(mdbg_ctx* ctx, double* ms);

/* ---- the resident reads threaded through the unitig graph ----------------------------------------------------------------------
 * Which unitigs, in which order and orientation, does each read walk?  The call works on the context's CURRENT unitig list (the list of the last
 * mdbg_graph_unitigs* / mdbg_graph_simplify* call), the node table that list was built from, and the resident sketch store; it keeps no new data and leaves the node
 * table, the edge list, the unitig list, the contig result and the component result as they are.  SINGLE GPU ONLY.
 *
 * Definition:
 *   READS are addressed by their slot in the store, r = 0 .. n - 1, the order of mdbg_sketch_view's d_read_offsets; ordinal[] gives a read's ordinal (its batch's
 *   first_read_ordinal plus its position in the batch).  A read with n minimizers has W = n - k + 1 WINDOWS if n > k, else none (src/main.rs:756-759, strictly more
 *   than k); window w covers minimizers w .. w + k - 1.  Its canonical key and its `rev` flag are KmerVec::normalize's: a window equal to its reverse counts as reversed.
 *   Window w is PLACED iff its key is a row of the current node table (abundance filter as --read_stats: min_abundance == 1 or (u16)count >= (u16)min_abundance) and that
 *   row's `index` occurs as node[e] of an entry e of the current list (after a simplify schedule some rows occur in no entry; an index occurs in at most one entry: the
 *   unitigs partition the surviving nodes).  For a placed window: unitig u = the unitig that holds e, entry j = e - offsets[u], strand s = rev XOR (ori[e] == '-');
 *   s = 0: the read walks the unitig in walk order.
 *   A STEP is a maximal run of consecutive placed windows w, w + 1, ... of one read with the same u and the same s whose j advances by +1 (s = 0) or by -1 (s = 1);
 *   on a CIRCULAR unitig of m entries the successor is taken mod m, so a read that goes round a ring more than once is ONE step with n_windows > m; a linear unitig
 *   never continues onto itself.  A window that is not placed belongs to no step and ends a run.  Step p is the record first_window[p], step_windows[p] (its number
 *   of windows), unitig[p], first_entry[p] (the j of its first window), strand[p]; the steps of read first_read + q are [step_offsets[q], step_offsets[q + 1]), in
 *   window order.
 *   Per unitig of the list: support_windows[u] = placed windows on u, support_steps[u] = steps on u, over the reads of the call's range.  Everything is an integer sum
 *   or a position of one scan: two calls give identical arrays, nothing depends on scheduling.
 *   n_reads = reads in the range, n_windows / n_placed / n_steps = their windows, placed windows and steps; read_windows[q] = W of read first_read + q.
 * Range: reads [first_read, first_read + max_reads) (max_reads = 0: to the end).  The temporaries are 9 bytes and the step arrays another 17 bytes per minimizer index of
 * the range, so the range bounds them.  first_read >= the number of reads: MDBG_OK with zero counts, which ends a caller's loop.  The step lists of the ranges of a
 * partition, concatenated, are the whole call's; their support arrays add up to the whole call's.
 * Invariant: over the whole store, and while no abundance has wrapped its u16, support_windows[u] == kc_sum[u] for every unitig — an abundance is a count of windows.
 * mdbg_graph_read_paths: HOST arrays; mdbg_graph_read_paths_device: DEVICE arrays.  They belong to the context until its next read-path call or mdbg_destroy and share
 * memory with no other result.  The number of kernel launches is fixed; the device variant waits for the device ONCE (the three counts and the defect flag in one
 * read-back) when the range starts and ends where batches do — the whole store always does —, otherwise once more, up front, for the range's two offsets.
 * mdbg_read_paths_ms: device time of the last read-path call (HIP events; 0 if it launched nothing).
 * MDBG_E_STATE: no current unitig list (an edge, finalize, ingest, rewind or reset call ended it), the node table is not current, or a routed / partitioned context;
 * MDBG_E_PARAM: a null pointer.  MDBG_E_CAPACITY: a list of 2^30 entries or more, or a range of 2^32 minimizers or more.  An empty context or an empty list gives MDBG_OK with every count zero (n_reads included) and no arrays.  MDBG_E_DEVICE: a list entry
 * whose node index is not a row of the table, a probe that ran past the table's capacity, or a solid slot that is no row — the device sets a flag and never indexes
 * outside or spins. */
typedef struct mdbg_read_path_list {
    uint64_t first_read, n_reads, n_windows, n_placed, n_steps, n_unitigs;
    const uint64_t* ordinal; const uint32_t* read_windows;      /* n_reads: the read's ordinal, its number of windows W */
    const uint64_t* step_offsets;                      /* n_reads + 1 */
    const uint32_t* first_window; const uint32_t* step_windows; const uint32_t* unitig; const uint32_t* first_entry; const uint8_t* strand;      /* n_steps */
    const uint64_t* support_windows; const uint64_t* support_steps;      /* n_unitigs */
} mdbg_read_path_list;
int mdbg_graph_read_paths(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out);
int mdbg_graph_read_paths_device(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_read_path_list* out);
int mdbg_read_paths_ms(mdbg_ctx* ctx, double* ms);

/* ---- read support per junction: the reads that cross each unitig edge, and the crossings no edge explains ----------------------------
 * An edge record of the graph does not come from a read: two nodes get an L line when they share a normalized (k-1)-mer, whether or not a read ever went from one to
 * the other.  This call counts, per edge record of the CURRENT unitig list, the resident reads that cross it, and lists the places where reads cross without a
 * record.  It works on what mdbg_graph_read_paths works on — the current unitig list, the node table that list was built from, the resident sketch store —, with the
 * same state requirements and the same range of reads [first_read, first_read + max_reads) (max_reads = 0: to the end).  SINGLE GPU ONLY.
 *
 * Definition.  Windows, PLACED, unitig u, entry j and strand s are those of mdbg_graph_read_paths; m(u) = offsets[u + 1] - offsets[u] is the entry count of unitig u.
 *   A VERTEX is (u, j, s); vertices are ordered by (u, j, s), which is the order of 2 * (offsets[u] + j) + s.
 *   The MIRROR of the ordered pair (x, y) is ((y.u, y.j, 1 - y.s), (x.u, x.j, 1 - x.s)).  The KEY of a pair is the smaller of the pair and its mirror, compared
 *   lexicographically on (x, y).
 *   An ADJACENT PAIR is windows w and w + 1 of one read, both placed; n_adjacent counts them over the range.
 *   A LINK is an adjacent pair x -> y with the same u, the same s, and y.j == x.j + 1 (s = 0) or y.j == x.j - 1 (s = 1), taken WITHOUT wrapping; n_links counts them.
 *   A CROSSING is every other adjacent pair — the wrap m - 1 -> 0 (s = 0) or 0 -> m - 1 (s = 1), which mdbg_graph_read_paths treats as the continuation of a step on
 *   a circular unitig, included.  n_crossings = n_adjacent - n_links.
 *   The key of EDGE RECORD r = (n1, o1, n2, o2) of the list's `edges` is the key of the pair x = (n1, o1 == '+' ? m(n1) - 1 : 0, o1 == '-'),
 *   y = (n2, o2 == '+' ? 0 : m(n2) - 1, o2 == '-').  A record and its mirror record have the same key, so do duplicate records; the closing record u + u + of a
 *   circular unitig has the key of its wrap.
 *   support[r], n_records entries parallel to the list's edge arrays, is the number of crossings in the range whose key is the key of record r: records with equal
 *   keys carry equal counts.  n_explained is the number of crossings whose key is some record's key.
 *   The other crossings are MISSING.  They are returned as their distinct keys in ascending key order, n_missing of them: missing_unitig1[], missing_entry1[],
 *   missing_strand1[] (x) and missing_unitig2[], missing_entry2[], missing_strand2[] (y), with missing_count[] the crossings on that key; n_missing_crossings is the
 *   sum of missing_count[].
 *   Everything is an integer sum or a position of a sort or a scan: two calls give identical arrays, nothing depends on scheduling.
 * Invariants: n_explained + n_missing_crossings == n_crossings; n_links + n_crossings == n_adjacent.  On a plain list (mdbg_graph_unitigs) built on edges of presimp 0,
 * n_missing == 0: consecutive windows share a (k-1)-mer, so their arc exists, and it is an interior link or both of its ends are unitig ends.  Against the read-path
 * result of the same range: n_links + wraps == n_placed - n_steps, with `wraps` the ring wraps inside steps (from first_entry, step_windows and strand of the steps
 * on circular unitigs).
 * Ranges: over the ranges of a partition of the reads the support arrays add up to the whole call's, the missing lists merge by key (counts added) into the whole
 * call's, and n_reads, n_adjacent, n_links, n_crossings, n_explained and n_missing_crossings add up.  first_read >= the number of reads: MDBG_OK with zero counts,
 * which ends a caller's loop `first_read += n_reads`.  The temporaries are 25 bytes per minimizer index of the range (the place codes 4, the keys of the missing
 * crossings and their sorted copy 16, head flags 1, positions 4) beside the sort's own, and the missing columns are sized for their worst case, another 26 bytes per
 * index, because their number is known only on the device: the range bounds both.  Per edge record the call takes 32 bytes of temporaries and 8 of result.
 * mdbg_graph_junctions: HOST arrays; mdbg_graph_junctions_device: DEVICE arrays.  They belong to the context until its next junction call, its next simplify call with an EDGES
 * step or mdbg_destroy and share memory with no other result — a read-path result the caller holds is untouched —, and the call leaves the node table, the edge list, the unitig list and the contig,
 * component and read-path results as they are.  The number of kernel launches is fixed; the device variant waits for the device ONCE (all counts and the defect flag
 * in one read-back) when the range starts and ends where batches do, otherwise once more, up front, for the range's two offsets.
 * mdbg_junctions_ms: device time of the last junction call (HIP events; 0 if it launched nothing); after a simplify call with EDGES steps, the device time
 * of their junction stages, summed.
 * MDBG_E_STATE: no current unitig list, the node table is not current, or a routed / partitioned context; MDBG_E_PARAM: a null pointer; MDBG_E_CAPACITY: the bounds of
 * the read paths (2^30 entries, 2^32 minimizers in the range) or 2^32 edge records; MDBG_E_DEVICE: the defect flags of the read paths, or an edge record that names a
 * unitig outside the list.  An empty context, an empty list or first_read >= the number of reads gives MDBG_OK with every count zero (n_records included) and no
 * arrays.  A list with no edge records and a non-empty range is ordinary: n_records == 0 and every crossing is missing. */
typedef struct mdbg_junction_list {
    uint64_t first_read, n_reads, n_adjacent, n_links, n_crossings, n_explained, n_missing_crossings, n_records, n_missing;
    const uint64_t* support;                                                                                  /* n_records */
    const uint32_t* missing_unitig1; const uint32_t* missing_entry1; const uint8_t* missing_strand1;          /* n_missing */
    const uint32_t* missing_unitig2; const uint32_t* missing_entry2; const uint8_t* missing_strand2;          /* n_missing */
    const uint64_t* missing_count;                                                                            /* n_missing */
} mdbg_junction_list;
int mdbg_graph_junctions(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_junction_list* out);
int mdbg_graph_junctions_device(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_junction_list* out);
int mdbg_junctions_ms(mdbg_ctx* ctx, double* ms);

/* ---- transits: the reads that span a unitig end to end, and the repeats they resolve ------------------------------------------------
 * A repeat longer than k - 1 minimizers is a unitig of its own with several ways in and several ways out, and every one of its edge records may be well supported:
 * the junction support cannot say which entrance goes with which exit.  A read that enters the unitig over one record, walks all of it and leaves over another
 * can.  This call lists, per unitig of the CURRENT list, every (entrance, exit) pair the resident reads take through it, with counts, and says per unitig whether
 * those pairs match its entrances to its exits one to one.  It works on what mdbg_graph_junctions works on, with the same state requirements, the same range of reads
 * [first_read, first_read + max_reads) (max_reads = 0: to the end), the same capacity bounds and the same defect flags.  It changes nothing: duplicating a resolved
 * unitig is the business of a simplify step (MDBG_SIMPLIFY_REPEATS, mdbg_graph_simplify above), which runs this stage on the list it decides against.  SINGLE GPU ONLY.
 *
 * Definition.  Windows, PLACED, vertex (u, j, s), pair, MIRROR, KEY, LINK, CROSSING, the key of an edge record and m(u) are those of mdbg_graph_junctions.  A crossing
 * is EXPLAINED iff its key is some record's key.
 *   A TRANSIT is two explained crossings of one read, c = x -> y at windows (w, w + 1) and c' = x' -> y' at windows (w', w' + 1) with w < w', such that every window
 *   w + 1 .. w' is placed and every adjacent pair strictly between the two crossings is a link (w' = w + 1: y and x' are the same window).  An unplaced window, a
 *   crossing whose key is no record's key, or the end of the read ends the chain.  Consecutive explained crossings overlap: a read with crossings c1, c2, c3 in an
 *   unbroken chain gives the transits (c1, c2) and (c2, c3).
 *   Consequence: y and x' lie on one unitig u with one strand s, y on the end the read enters by and x' on the end it leaves by, and w' - w == m(u): the read walks
 *   all of u.  (A record's pair ends on an end of its unitig and links never wrap.  The device checks it on every transit; a chain that breaks it is a defect.)
 *   CANONICAL FORM: if s == 1, (c, c') is replaced by (mirror(c'), mirror(c)), the same walk read from the other strand.  The in-pair is then p -> (u, 0, 0) and
 *   the out-pair (u, m(u) - 1, 0) -> q.  The TRANSIT KEY is (u, p, q), ordered by u, then p, then q in the junctions' vertex order; reads of both strands fall together.
 *   Per distinct key, in key order, n_transits rows: unitig[] = u; in_unitig[], in_entry[], in_strand[] = p; out_unitig[], out_entry[], out_strand[] = q;
 *   in_record[] / out_record[] = the smallest record number whose key is the key of the in-pair / of the out-pair; count[] = the transits of the range with that key.
 *   Per unitig u of the list, n_unitigs entries: n_in[u] = the distinct keys among the records' pairs and their mirrors whose pair has target (u, 0, 0);
 *   n_out[u] likewise for source (u, m(u) - 1, 0); passes[u] = the sum of count[] over u's keys; verdict[u] for the call's min_support >= 1, the first test that applies:
 *     MDBG_TRANSIT_PLAIN       n_in < 2 or n_out < 2;
 *     MDBG_TRANSIT_SELF        some record has n1 == n2 == u;
 *     MDBG_TRANSIT_RESOLVED    n_in == n_out, n_in equals the number of u's keys with count >= min_support (the STRONG ones), and the strong keys have pairwise different
 *                              p and pairwise different q: a perfect matching of entrances and exits.  Weak keys do not block, as weak records do not in an EDGES step;
 *     MDBG_TRANSIT_UNRESOLVED  otherwise.
 *   n_crossings and n_explained are the junctions'; n_passes is the sum of count[]; n_transits the number of distinct keys; n_repeats the unitigs with n_in >= 2 and
 *   n_out >= 2; n_resolved the RESOLVED ones.  n_in, n_out and the SELF test depend on the records alone, not on the range.
 *   Everything is an integer sum or a position of a sort or a scan: two calls give identical arrays, nothing depends on scheduling.
 * Invariants: the sum of passes[] is n_passes; passes[u] <= support_steps[u] of the read paths of the same range for every LINEAR unitig (a transit's walk is a
 * step of its own; on a circular unitig one step that wraps r times holds r - 1 transits, so the bound does not hold there);
 * count[i] <= min(support[in_record[i]], support[out_record[i]]) of the junctions of the same range, with the support of a pair that is its OWN MIRROR taken
 * twice (one such crossing closes a transit of strand 0 and opens one of strand 1 that fall on one key; no other crossing serves a key twice).
 * Ranges: over the ranges of a partition of the reads the rows merge by key (counts added) into the whole call's, passes[] add up, and n_reads, n_crossings,
 * n_explained and n_passes add up.  Verdicts, n_repeats and n_resolved belong to the range they were computed on; apply the rule to the merged counts for the whole.
 * The temporaries are 35 bytes per minimizer index of the range (the place codes 4, the kind of each pair 1, the transit keys 12 and their second copy 12, head
 * flags 1, positions 4, direction bits 1) beside the sorts' own, and the row columns are sized for their worst case, another 38 bytes per index, because their number
 * is known only on the device: the range bounds both.  Per edge record the call takes 40 bytes of temporaries, per unitig 6 bytes of temporaries and 17 of result.
 * mdbg_graph_transits: HOST arrays; mdbg_graph_transits_device: DEVICE arrays.  They belong to the context until its next transit call or mdbg_destroy and share memory
 * with no other result: a read-path, junction, component or contig result the caller holds is untouched by the call, and a transit result survives a junction call
 * and a simplify call.  The number of kernel launches is fixed; the device variant waits for the device ONCE (all counts and the defect flag in one read-back) when
 * the range starts and ends where batches do, otherwise once more, up front, for the range's two offsets.
 * mdbg_transits_ms: device time of the last transit call (HIP events; 0 if it launched nothing).
 * MDBG_E_PARAM: min_support == 0 or a null pointer; MDBG_E_STATE, MDBG_E_CAPACITY: as mdbg_graph_junctions; MDBG_E_DEVICE: its defect flags, or a chain of two
 * explained crossings that does not walk all of one unitig.  An empty context, an empty list or first_read >= the number of reads gives MDBG_OK with every count zero
 * (n_unitigs included) and no arrays. */
enum { MDBG_TRANSIT_PLAIN = 0, MDBG_TRANSIT_RESOLVED = 1, MDBG_TRANSIT_UNRESOLVED = 2, MDBG_TRANSIT_SELF = 3 };
typedef struct mdbg_transit_list {
    uint64_t first_read, n_reads, n_crossings, n_explained, n_passes, n_transits, n_unitigs, n_repeats, n_resolved;
    const uint32_t* unitig;                                                                          /* n_transits */
    const uint32_t* in_unitig; const uint32_t* in_entry; const uint8_t* in_strand;                   /* n_transits */
    const uint32_t* out_unitig; const uint32_t* out_entry; const uint8_t* out_strand;                /* n_transits */
    const uint32_t* in_record; const uint32_t* out_record; const uint64_t* count;                    /* n_transits */
    const uint32_t* n_in; const uint32_t* n_out; const uint64_t* passes; const uint8_t* verdict;     /* n_unitigs */
} mdbg_transit_list;
int mdbg_graph_transits(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, uint64_t min_support, mdbg_transit_list* out);
int mdbg_graph_transits_device(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, uint64_t min_support, mdbg_transit_list* out);
int mdbg_transits_ms(mdbg_ctx* ctx, double* ms);

/* ---- alignments: the steps of the read paths chained over edge records, with base coordinates; queries that are not resident; GAF lines: include/mdbg_align.h ---- */

/* ---- multi-GPU, second mode: replicated sketches, partitioned table ----------------------------------------
 * Within one node the sketch is much more compact than the k-min-mers cut from it (every minimizer sits in k windows),
 * so the ranks may exchange SKETCHES instead (one all-gather), each rank then windows the global sketch but inserts only
 * the k-min-mers it owns.  Ownership is an O(1) function of the canonical key (its two ends and its middle), the table,
 * insertion and finalize are the single-GPU ones, and nothing is approximate.  DbgEntry.index needs the first sightings
 * of all ranks: mdbg_finalize_begin exposes this rank's first-sighting / solid bitmaps over the (identical on every
 * rank) global sketch; the driver sums them across ranks (bits are disjoint) and mdbg_finalize_end emits the rows. */
int mdbg_set_partition(mdbg_ctx* ctx, uint32_t world, uint32_t rank);   /* before the first insertion */
typedef struct mdbg_sketch_store {
    uint64_t n_minimizers, n_reads;
    const uint64_t* d_hashes;        /* [n_minimizers] DEVICE */
    const uint32_t* d_positions;     /* [n_minimizers] raw position relative to the read */
    const uint64_t* d_read_offsets;  /* [n_reads + 1] first minimizer of every read */
} mdbg_sketch_store;
int mdbg_sketch_view(mdbg_ctx* ctx, mdbg_sketch_store* out);  /* the resident store (valid until the next sketch/ingest/reset) */
/* Append an already computed sketch (DEVICE arrays, e.g. another rank's mdbg_sketch_view): n_reads reads whose minimizers
 * are hashes/positions[read_offsets[r] .. read_offsets[r+1]).  Counterpart of mdbg_sketch_device without the kernel. */
int mdbg_ingest_sketch(mdbg_ctx* ctx, const uint64_t* d_hashes, const uint32_t* d_positions, const uint64_t* d_read_offsets,
                       uint64_t n_reads, uint64_t first_read_ordinal);
/* Zero-copy variant for receives that can write straight into the resident store (RCCL recv, peer copies):
 *   mdbg_store_reserve   sizes the store up front (total minimizers / reads it will hold), so that it never has to move;
 *   mdbg_sketch_reserve  appends an UNCOMMITTED region of n_minimizers entries and returns where to write its hashes and
 *                        positions (DEVICE pointers; they stay valid because the store refuses to grow, MDBG_E_STATE, while
 *                        regions are pending); *region identifies it;
 *   mdbg_sketch_commit   registers [region, region + n_minimizers) - or any part of a reserved region - as the sketch of
 *                        n_reads reads; d_read_offsets are relative to `region` ([0] = 0, [n_reads] = n_minimizers, checked
 *                        on the device: a violation is reported as MDBG_E_PARAM by the next mdbg_insert_resident).  The
 *                        call is stream-ordered: the offsets buffer must stay alive until the next synchronising call.
 *                        owned_windows: see mdbg_owner_counts.
 *   mdbg_last_batch      describes the batch registered last (e.g. the one mdbg_sketch_device just produced), with DEVICE
 *                        pointers to its part of the store: what a rank sends to its peers.  Synchronises the context's
 *                        stream, so the arrays may be read from any other stream afterwards. */
int mdbg_store_reserve(mdbg_ctx* ctx, uint64_t n_minimizers_total, uint64_t n_reads_total);
int mdbg_sketch_reserve(mdbg_ctx* ctx, uint64_t n_minimizers, uint64_t** d_hashes, uint32_t** d_positions, uint64_t* region);
int mdbg_sketch_commit(mdbg_ctx* ctx, uint64_t region, uint64_t n_minimizers, const uint64_t* d_read_offsets, uint64_t n_reads,
                       uint64_t first_read_ordinal, uint64_t owned_windows);
/* Windows of the batch registered last, counted per owning rank (counts[world], HOST): computed once by the rank that
 * sketched the batch and shipped with it (mdbg_sketch_commit's owned_windows = counts[receiver]; UINT64_MAX = unknown), so
 * that the receivers size their tables without re-counting a foreign sketch.  When world equals this context's partition,
 * the call also records the context's own share for its own batch.  The counts are verified against what is actually
 * inserted (MDBG_E_PARAM from mdbg_insert_resident on a mismatch). */
int mdbg_owner_counts(mdbg_ctx* ctx, uint32_t world, uint64_t* counts);
/* Owner LISTS: like mdbg_owner_counts, and in addition the windows themselves, bucketed by owning rank: d_lists (DEVICE, library-owned
 * until the next call of this function) holds counts[0] entries for rank 0, then counts[1] for rank 1, ...; an ENTRY is a pair of
 * uint32_t: the index of the window's first minimizer and the index of its read, both relative to the batch (so rank r's bucket starts
 * at d_lists + 2 * (counts[0] + ... + counts[r-1]) and is 8 * counts[r] bytes).  The sender ships bucket r to rank r with the sketch
 * (8 bytes per window) and the receiver registers it with mdbg_sketch_commit_listed (n_list = number of entries): it then inserts
 * exactly its windows — no scan of the foreign sketch, no minimizer -> read map built for it — so the per-rank work does not grow with
 * the number of ranks.  world <= 64.  Buckets are ordered by spans of 2048 window starts (any order inside a span); every entry is
 * verified at insertion (range, read, ownership, and the total count: MDBG_E_PARAM from mdbg_insert_resident on a mismatch).  The list
 * is copied by mdbg_sketch_commit_listed: the caller's buffer may be reused once the context's stream has passed the call (mdbg_sync). */
int mdbg_owner_lists(mdbg_ctx* ctx, uint32_t world, uint64_t* counts, const uint32_t** d_lists);
int mdbg_sketch_commit_listed(mdbg_ctx* ctx, uint64_t region, uint64_t n_minimizers, const uint64_t* d_read_offsets, uint64_t n_reads,
                              uint64_t first_read_ordinal, const uint32_t* d_list, uint64_t n_list);
typedef struct mdbg_batch_info {
    uint64_t store_offset, n_minimizers, first_slot, n_reads, first_read_ordinal;
    const uint64_t* d_hashes;        /* [n_minimizers] */
    const uint32_t* d_positions;     /* [n_minimizers] */
    const uint64_t* d_read_offsets;  /* [n_reads + 1], absolute: subtract store_offset for offsets relative to the batch */
} mdbg_batch_info;
int mdbg_last_batch(mdbg_ctx* ctx, mdbg_batch_info* out);
int mdbg_finalize_begin(mdbg_ctx* ctx, uint64_t** d_bm_first, uint64_t** d_bm_solid, uint64_t* n_words);
/* out: DEVICE pointers, this rank's nodes in table order; d_row[i] = global row (position in index order);
 * out->n_distinct and *n_nodes_global are the totals over all ranks (from the merged bitmaps). */
int mdbg_finalize_end(mdbg_ctx* ctx, mdbg_nodes* out, const uint64_t** d_row, uint64_t* n_nodes_global);

/* Wait for all device work queued by ctx. */
int mdbg_sync(mdbg_ctx* ctx);
/* Plain copies between host memory and device buffers handed out by / given to this library. */
int mdbg_copy_to_host(mdbg_ctx* ctx, void* dst, const void* d_src, uint64_t nbytes);
int mdbg_copy_to_device(mdbg_ctx* ctx, void* d_dst, const void* src, uint64_t nbytes);

/* Synthetic HiFi-shaped reads (counter-based, integer-only generator; the same bytes can be regenerated
 * on the CPU, see rust_mdbg_amd/synth.py).  Fills library-owned DEVICE buffers. */
typedef struct mdbg_synth_params {
    uint64_t seed;
    uint64_t genome_len;
    uint64_t n_reads;
    uint32_t mean_len, sd_len, min_len, max_len;
    uint32_t err_ppm;           /* per-base error rate in parts per million, split sub/ins/del 1:1:1 */
    uint32_t reserved;
} mdbg_synth_params;
int mdbg_synth_reads_device(mdbg_ctx* ctx, const mdbg_synth_params* sp, uint64_t first_read,
                            const uint8_t** d_bases, const uint64_t** d_offsets, uint64_t* n_bases);

/* Measurement hook (scratch/measure_rank_w8.py; no counterpart in the reference): milliseconds the multi-GPU layer's sender (out[0]) and receiver (out[1]) spend on the
 * segments of the batch registered last for `world` ranks; counts / d_lists as mdbg_owner_lists returned them, `skip` = the bucket that ships nothing;
 * out[2] = list entries, out[3] = hashes packed. */
int mdbg_dbg_segments_ms(mdbg_ctx* ctx, uint32_t world, uint32_t skip, const uint64_t* counts, const uint32_t* d_lists, double* out);

/* ---- test hooks ------------------------------------------------------------------------------------
 * MDBG_GUARD (environment, read once): every device block of the library is an allocation of its own, exactly as large as the stage asked for, poisoned
 * with 0xA5 and fenced by two bands of 4096 bytes, one in front and one behind, inside the same allocation.  A kernel that writes up to 4 KiB outside its buffer
 * damages a band instead of a neighbour or the slack of the buffer.  Writes only: a read outside a block leaves no trace.  Unset, nothing changes.
 * mdbg_guard_check: waits for the device, compares both bands of every live block (and repairs a damaged one, so that it counts once) and returns the number of
 * damaged bands found so far, those found when a block was given back included; *n_blocks / *n_bytes <- live blocks and payload bytes looked at (either may be
 * NULL).  0 and zeros when MDBG_GUARD is unset.
 * mdbg_guard_report: the first violation as text, "block of 1234 bytes: byte +3 behind the end (5 damaged)" or "...: byte -8 in front (8 damaged)": the size names the
 * request, the offset the damaged byte next to the payload.  "" when there is none.  Valid until the next call.
 * mdbg_guard_selftest: plants one byte behind the end and one in front of a 1000-byte block of its own (inside that block's allocation), expects each to be counted
 * once and named, and takes both out of the count again.  0 = the guard works, -1 = MDBG_GUARD is unset, > 0 = the step that failed. */
uint64_t mdbg_guard_check(uint64_t* n_blocks, uint64_t* n_bytes);
const char* mdbg_guard_report(void);
int mdbg_guard_selftest(void);

#ifdef __cplusplus
}
#endif
#endif /* MDBG_HIP_H */
