/* mdbg_align.h — alignments: reads and query sequences walked through the unitig graph, with base coordinates, and their GAF lines.
 *
 * The calls on a context (mdbg_graph_alignments*, mdbg_graph_align_batch*, mdbg_alignments_ms) are part of libmdbg_hip, the writer (mdbg_gaf_append) of
 * libmdbg_emit; they are declared here, in a header of their own beside mdbg_hip.h and mdbg_emit.h, which this one includes.  Plain C ABI.
 */
#ifndef MDBG_ALIGN_H
#define MDBG_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#include "mdbg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- alignments: the steps of the read paths chained over edge records, with base coordinates -----------------------------------------------
 * A read path (mdbg_graph_read_paths, mdbg_hip.h) is a list of steps in window and entry numbers.  This call says which consecutive steps are ONE walk over an
 * existing edge record and which are a jump, and gives every walk its coordinates in bases, on the read and on the path of unitigs: what a GAF line holds.  It works
 * on what mdbg_graph_junctions works on — the CURRENT unitig list with its edge records, the node table that list was built from, the resident sketch store —, with
 * the same state requirements, the same range of reads [first_read, first_read + max_reads) (max_reads = 0: to the end), the same capacity bounds and error codes.
 * A list that holds copies (a REPEATS or NESTED step) answers MDBG_E_STATE, as the other public read-evidence calls do.  SINGLE GPU ONLY.
 *
 * Definition.  Windows, PLACED, STEP and the step columns are those of mdbg_graph_read_paths; vertex, pair, KEY, LINK, CROSSING, EXPLAINED, the key of an edge record
 * and m(u) those of mdbg_graph_junctions and mdbg_graph_transits.
 *   STEPS  are the steps of mdbg_graph_read_paths over the same range, with the same columns (ordinal, read_windows, step_offsets, first_window, step_windows, unitig,
 *     first_entry, strand): the call runs that stage, fills the context's read-path result, and the step columns of this list ARE that result's arrays.
 *   CHAINED  Two consecutive steps p, p + 1 of one read are chained iff first_window[p + 1] == first_window[p] + step_windows[p] (no unplaced window lies between
 *     them) and the adjacent pair (last window of p, first window of p + 1) is EXPLAINED.  That pair is always a crossing, never a link, because steps are maximal.
 *     step_record[p + 1] is then the smallest record number whose key is the pair's key; step_record[p] == 0xFFFFFFFF on a step that is not chained to the one in
 *     front of it.  n_chained counts the chained steps.
 *   ALIGNMENT  A maximal run of chained steps.  The alignments partition the steps in order: alignment a holds the steps [aln_step_offsets[a],
 *     aln_step_offsets[a + 1]), aln_step_offsets[n_alignments] == n_steps; the alignments of read first_read + q are [aln_offsets[q], aln_offsets[q + 1]).
 *   QUERY SIDE, in the raw positions of the store (d_positions of mdbg_sketch_view; on a context that compresses homopolymers these are positions in the compressed
 *     read), with w0 / w1 the first / last window of the alignment:
 *       aln_windows = the sum of its step_windows;  query_begin = pos[w0];  query_end = pos[w1 + k - 1] + l   (the end of a node's sequence, src/main.rs:778).
 *   PATH SIDE, in bases.  For entry e of the list (global number offsets[u] + j) whose node is row r of the table: E(e) = dst_offset[e] + len[e], the end of the node's
 *     sequence inside the unitig's, and B(e) = E(e) - (src_end[r] - src_start[r]), clamped at 0, its begin.  (NOT seqlen[r]: that column is the reference's
 *     read_offsets.2, last position + 1 - first position + 1 (src/main.rs:778), which is l - 2 short of the node's sequence [first position, last position + l).)
 *     The PATH is the list of unitig occurrences: each step contributes its unitig 1 + wraps times, wraps = the ring closures inside the step,
 *       strand 0: (first_entry + step_windows - 1) div m(u);  strand 1: (m(u) - 1 - first_entry + step_windows - 1) div m(u);  0 on a linear unitig.
 *     Two consecutive occurrences overlap: between two steps over step_record; inside a wrapping step over the ring's closing record (the smallest record whose
 *     key is the key of the wrap (u, m - 1, 0) -> (u, 0, 0)).  The BASE OVERLAP of record r is overlap[r] + l - 2: a record's overlap is counted on seqlen
 *     (mdbg_graph_edges: n1.seqlen - shift), so it is the same l - 2 short of the bases the two sequences share; the GFA's L lines print overlap[r] as it is.
 *      length[] of a CIRCULAR unitig is the sum of its entries' len like any
 *     other: the first entry contributes all of its node, so the bases the closing record overlaps are INCLUDED once at the end of the sequence and once at its
 *     start, and a second turn starts length[u] - (its base overlap) bases after the first.
 *       path_length = the sum of length[u] over the occurrences minus the sum of those base overlaps;
 *       path_begin  = B(first entry) on strand 0, length[u] - E(first entry) on strand 1, at the first window's entry on the first occurrence;
 *       path_end    = path_length - tail, tail = length[u] - E(e) on strand 0, B(e) on strand 1, at the last window's entry e on the last occurrence.
 *     With error-free reads the bases [path_begin, path_end) of the path's sequence — the unitigs' sequences joined with those base overlaps, an occurrence of strand 1
 *     reverse-complemented — are the bases [query_begin, query_end) of the read.
 *   n_reads, n_windows, n_placed, n_steps are the read paths'; n_wraps is the sum of wraps over the steps.
 *   Everything is an integer sum or a position of a sort or a scan: two calls give identical arrays, nothing depends on scheduling.
 * Invariants: n_alignments == n_steps - n_chained.  Against mdbg_graph_junctions of the same range: n_explained == n_chained + n_wraps.  On a plain list built on
 * edges of presimp 0 n_missing == 0 there, so the alignments of a read are separated by unplaced windows only.
 * Ranges: over the ranges of a partition of the reads the step and alignment columns concatenate (the offsets shifted by what came before) and the counters add up.
 * first_read >= the number of reads: MDBG_OK with zero counts.  Per minimizer index of the range the call takes, beside the read paths' 9 + 17 bytes, 9 bytes of
 * temporaries, 4 of step_record and 44 of alignment columns, sized for the worst case; per edge record 24 bytes of temporaries.
 * mdbg_graph_alignments: HOST arrays; mdbg_graph_alignments_device: DEVICE arrays.  The alignment columns belong to the context until its next alignment call or
 * mdbg_destroy; the step columns are the read-path result and end with it (the next read-path or alignment call).  The call leaves the node table, the edge list, the
 * unitig list and the component, contig, junction and transit results as they are: it uses the context's one placement scratch, which holds no result.  The number of
 * kernel launches is fixed; the device variant waits for the device ONCE (all counts and the defect flag in one read-back) when the range starts and ends where
 * batches do, otherwise once more, up front, for the range's two offsets.
 * mdbg_alignments_ms: device time of the last alignment call (HIP events; 0 if it launched nothing), the read-path stage inside it included; mdbg_read_paths_ms
 * reports the same figure after such a call.
 * MDBG_E_STATE, MDBG_E_PARAM, MDBG_E_CAPACITY: as mdbg_graph_junctions.  MDBG_E_DEVICE: its defect flags; a record that is needed is absent or outside the list (the
 * closing record of a ring some step wraps); an entry without a row — the device sets a flag and never indexes outside a buffer.  An empty context, an empty list or
 * first_read >= the number of reads gives MDBG_OK with every count zero and no arrays. */
typedef struct mdbg_alignment_list {
    uint64_t first_read, n_reads, n_windows, n_placed, n_steps, n_chained, n_alignments, n_wraps, n_unitigs;
    const uint64_t* ordinal; const uint32_t* read_windows;      /* n_reads */
    const uint64_t* step_offsets; const uint64_t* aln_offsets;  /* n_reads + 1 */
    const uint32_t* first_window; const uint32_t* step_windows; const uint32_t* unitig; const uint32_t* first_entry; const uint8_t* strand; const uint32_t* step_record;  /* n_steps */
    const uint64_t* aln_step_offsets;                           /* n_alignments + 1 */
    const uint32_t* aln_windows; const uint32_t* query_begin; const uint32_t* query_end;                          /* n_alignments */
    const uint64_t* path_length; const uint64_t* path_begin; const uint64_t* path_end;                            /* n_alignments */
} mdbg_alignment_list;
int mdbg_graph_alignments(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_alignment_list* out);
int mdbg_graph_alignments_device(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, mdbg_alignment_list* out);
int mdbg_alignments_ms(mdbg_ctx* ctx, double* ms);

/* ---- aligning a batch that is not resident --------------------------------------------------------------------------------------------------
 * The same for sequences that are NOT part of the graph's input (genes, a reference, another assembly's contigs): bases / offsets are HOST buffers as
 * mdbg_query_batch takes them.  The batch is sketched behind the resident store, the stage above runs over exactly that batch's reads, and the store and the
 * stats are rolled back on every way out: the node table, the unitig list, the resident sketches, mdbg_get_stats and every held result except the alignment and the
 * read-path result are unchanged afterwards.  Read q of the list is query q of the batch and ordinal[q] == q; first_read == 0.  Refusals: those of mdbg_query_batch
 * (a routed or partitioned context) and those of mdbg_graph_alignments.  A byte outside the alphabet answers MDBG_E_ALPHABET and does not poison the context; the
 * --lmer-counts filter applies as it does to a resident batch.  n_reads == 0: MDBG_OK with zero counts.
 * mdbg_graph_align_batch: HOST arrays; mdbg_graph_align_batch_device: DEVICE arrays. */
int mdbg_graph_align_batch(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, mdbg_alignment_list* out);
int mdbg_graph_align_batch_device(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, mdbg_alignment_list* out);

/* ---- GAF (libmdbg_emit) ---------------------------------------------------------------------------------------------------------------------
 * Appends the GAF lines of one alignment list (HOST arrays) to `path` (truncate != 0: the file is created or emptied first).  unitigs: the list the alignments were
 * made on (HOST arrays; offsets and circular are read); read_lengths[q] = the raw length of read first_read + q.  One line per alignment, 12 columns and two tags:
 *   qname = the read's ordinal in decimal (the reader hands out no names), qlen, qstart = query_begin, qend = query_end, strand `+`,
 *   path = the unitig occurrences, `>` on strand 0 and `<` on strand 1 in front of the name mdbg_emit_contigs_write_gfa prints (utg%07d + l / c), a ring walked
 *   w + 1 times listed w + 1 times, plen = path_length, pstart = path_begin, pend = path_end,
 *   column 10 = min(qend - qstart, pend - pstart), column 11 = max of the same two (a minimizer-space alignment has no base-level matches: the two columns bound
 *   the aligned block from below and above), mapq 255, nw:i:<aln_windows>, ns:i:<steps of the alignment>.
 * MDBG_E_IO: the file cannot be opened or a write fails; MDBG_E_PARAM: a null pointer, or a step that names a unitig outside the list. */
int mdbg_gaf_append(const char* path, int truncate, const mdbg_alignment_list* alignments, const mdbg_unitig_list* unitigs, const uint64_t* read_lengths);

#ifdef __cplusplus
}
#endif
#endif
