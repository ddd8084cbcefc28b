/* mdbg_chain.h — gapped chains: the alignments of one read joined across unplaced windows where the graph says the two sides belong together.
 *
 * The calls on a context (mdbg_graph_chains*, mdbg_graph_chain_batch*, mdbg_chains_ms) are part of libmdbg_hip, the writer (mdbg_gaf_append_chains) of
 * libmdbg_emit; they are declared here, in a header of their own beside mdbg_align.h, which this one includes.  Plain C ABI.
 */
#ifndef MDBG_CHAIN_H
#define MDBG_CHAIN_H

#include <stddef.h>
#include <stdint.h>

#include "mdbg_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- chains: consecutive alignments of one read joined over a bridge ---------------------------------------------------------------------------
 * An alignment (mdbg_graph_alignments, mdbg_align.h) ends wherever a window of the read is not placed: one wrong or lost minimizer unplaces up to k consecutive
 * windows and cuts the read in two.  This stage leaves the reads and the alignments as they are and says which consecutive alignments of a read are ONE walk with a
 * hole in it, because the graph joins the two sides at the right distance.  It runs the alignment stage over the same range of reads [first_read, first_read +
 * max_reads) (max_reads = 0: to the end) and then a handful of kernels over the alignments; `alignments` of the result IS that stage's list, and the context's
 * alignment and read-path results are this call's.  State requirements, refusals, capacity bounds and error codes are those of mdbg_graph_alignments; in
 * particular a list that holds copies (a REPEATS or NESTED step), or a routed or partitioned context, answers MDBG_E_STATE.  SINGLE GPU ONLY.
 *
 * Definition.  Windows, PLACED, the placement (u, j, s) of a window, m(u), KEY, the key of an edge record, the base overlap overlap[r] + l - 2 of record r, alignment
 * and occurrence are those of mdbg_align.h and mdbg_hip.h.  Parameters: max_skew (u32) and max_gap (u32, 0 = no limit).
 *   For two consecutive alignments a - 1 and a of the SAME read let x = (u_x, j_x, s_x) be the placement of the last window w_x of a - 1, y = (u_y, j_y, s_y) that of
 *   the first window w_y of a, and dw = w_y - w_x (>= 1).
 *   Candidate INSIDE  exists iff u_x == u_y, s_x == s_y and de_I >= 1, where de_I = j_y - j_x on strand 0 and j_x - j_y on strand 1.  There is no modulo: a ring's
 *     closure is the other candidate.
 *   Candidate RECORD  Let tail = the entries behind j_x in walk direction (m(u_x) - 1 - j_x on strand 0, j_x on strand 1) and head = the entries in front of j_y in
 *     walk direction (j_y on strand 0, m(u_y) - 1 - j_y on strand 1).  Take the pair of the last vertex of u_x in direction s_x and the first vertex of u_y in
 *     direction s_y: (u_x, s_x ? 0 : m - 1, s_x) -> (u_y, s_y ? m - 1 : 0, s_y).  The candidate exists iff the KEY of that pair is the key of an edge record of the
 *     list; de_R = tail + head + 1, and its record is the smallest record number with that key.  u_x == u_y is allowed: a ring's closing record, or a self-loop.
 *   BRIDGE  Of the candidates that exist take the one with the smaller |de - dw|; a tie goes to INSIDE.  a is BRIDGED to a - 1 iff dw >= 2 (an unplaced window lies
 *     between the two; a crossing on no record, dw == 1, is never bridged), |de - dw| <= max_skew, and max_gap == 0 or dw - 1 <= max_gap.  The candidate is chosen
 *     BEFORE the thresholds: the kind of a bridge does not depend on max_skew, and the set of bridged alignments is monotone in both parameters (a larger max_skew, or
 *     a larger or unlimited max_gap, bridges a superset).  Why skew: a substituted minimizer gives de == dw, a lost one de == dw + 1, a spurious one de == dw - 1;
 *     several errors inside one gap add up.
 *     bridge_record[a] = 0xFFFFFFFF when a is not bridged (always for the first alignment of a read), 0xFFFFFFFE for INSIDE, otherwise the record number;
 *     bridge_entries[a] = de of the bridge, 0 when not bridged.
 *     A gap that would need TWO OR MORE records — a whole short unitig lying inside the gap — is not bridged: neither candidate exists.
 *   CHAIN  A maximal run of bridged alignments of one read.  The chains partition the alignments in order: chain c holds the alignments [chain_aln_offsets[c],
 *     chain_aln_offsets[c + 1]), chain_aln_offsets[n_chains] == n_alignments; the chains of read first_read + q are [chain_offsets[q], chain_offsets[q + 1]).
 *       chain_windows = the sum of aln_windows;  chain_gap_windows = the sum of dw - 1 over its bridges;
 *       query_begin = that of its first alignment, query_end = that of its last.
 *     The PATH is the alignments' occurrence lists one behind the other, joined so: an INSIDE bridge MERGES the last occurrence in front of it and the first behind it
 *     into one (the same unitig, strand and turn); a RECORD bridge leaves them adjacent, overlapping by the record's base overlap.
 *       path_length = the sum of the alignments' path_length - the sum over INSIDE bridges of length[u_x] - the sum over RECORD bridges of the base overlap;
 *       path_begin  = the first alignment's;  path_end = path_length - (path_length - path_end) of the last alignment.
 *     The bases [path_begin, path_end) of the path and [query_begin, query_end) of the read agree outside the gaps; inside a gap their lengths may differ.
 *   Counters: n_bridges_inside, n_bridges_record, n_bridges = their sum, n_chains, n_gap_windows = the sum of chain_gap_windows.
 * Invariants: n_chains == n_alignments - n_bridges; the sum of chain_windows == n_placed; n_gap_windows <= n_windows - n_placed.
 * Ranges: over the ranges of a partition of the reads the columns concatenate (the offsets shifted by what came before) and the counters add up, as for alignments.
 * Everything is an integer sum or a position of a scan: two calls give identical arrays.
 * NOT done: a gap over two or more records; lists with copies; more than one GPU; bridges as evidence for junctions, transits or the REPEATS step.
 *
 * mdbg_graph_chains: HOST arrays; mdbg_graph_chains_device: DEVICE arrays.  The chain and bridge columns belong to the context until its next chain call or
 * mdbg_destroy; `alignments` is the alignment result (until the next alignment or chain call) and its step columns the read-path result.  Every other held result, the
 * node table, the edge list and the unitig list stay as they are.  The alignment stage's counts are on the host when the chain kernels are queued, so their buffers
 * and grids are sized by n_alignments.  The number of kernel launches is fixed: those of the alignment call, and behind them five memsets (one of them a single byte), four kernels and one
 * scan.  The call waits for the device ONCE more than the alignment call does, for the chain counts; with n_alignments == 0 it queues two memsets and does not wait.
 * mdbg_chains_ms: device time of the last chain call (HIP events; 0 if it launched nothing), the alignment stage inside it included; mdbg_alignments_ms reports that
 * stage's share after such a call.
 * MDBG_E_DEVICE beside the alignment call's: an alignment names a step, a unitig or a record outside its list — the device sets a flag and never indexes outside a
 * buffer.  An empty context, an empty list or first_read >= the number of reads gives MDBG_OK with every count zero and no arrays. */
#define MDBG_BRIDGE_NONE   0xFFFFFFFFu
#define MDBG_BRIDGE_INSIDE 0xFFFFFFFEu
typedef struct mdbg_chain_list {
    mdbg_alignment_list alignments;
    uint64_t n_bridges, n_bridges_inside, n_bridges_record, n_chains, n_gap_windows;
    const uint32_t* bridge_record; const uint64_t* bridge_entries;                                                 /* n_alignments */
    const uint64_t* chain_offsets;                                                                                 /* n_reads + 1 */
    const uint64_t* chain_aln_offsets;                                                                             /* n_chains + 1 */
    const uint32_t* chain_windows; const uint32_t* chain_gap_windows; const uint32_t* query_begin; const uint32_t* query_end;      /* n_chains */
    const uint64_t* path_length; const uint64_t* path_begin; const uint64_t* path_end;                            /* n_chains */
} mdbg_chain_list;
int mdbg_graph_chains(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out);
int mdbg_graph_chains_device(mdbg_ctx* ctx, uint64_t first_read, uint64_t max_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out);
int mdbg_chains_ms(mdbg_ctx* ctx, double* ms);

/* ---- chaining a batch that is not resident -----------------------------------------------------------------------------------------------------
 * mdbg_graph_align_batch with the chain stage behind it: the batch is sketched behind the resident store, aligned and chained, and the store and the stats are
 * rolled back on every way out.  Read q of the list is query q of the batch; refusals, MDBG_E_ALPHABET and n_reads == 0 as there.  Afterwards the alignment, the
 * read-path and the chain result are this call's; everything else is unchanged.
 * mdbg_graph_chain_batch: HOST arrays; mdbg_graph_chain_batch_device: DEVICE arrays. */
int mdbg_graph_chain_batch(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out);
int mdbg_graph_chain_batch_device(mdbg_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint32_t max_skew, uint32_t max_gap, mdbg_chain_list* out);

/* ---- GAF (libmdbg_emit) ------------------------------------------------------------------------------------------------------------------------
 * Appends the GAF lines of one chain list (HOST arrays) to `path`, as mdbg_gaf_append does for an alignment list: ONE LINE PER CHAIN, the same 12 columns —
 *   qname, qlen, qstart = the chain's query_begin, qend = its query_end, `+`, the chain's PATH with merged occurrences as defined above, plen = path_length,
 *   pstart = path_begin, pend = path_end, column 10 = min(qend - qstart, pend - pstart), column 11 = the max of the two, mapq 255 —
 * and four tags: nw:i:<chain_windows> (placed windows), ns:i:<steps of its alignments>, ng:i:<bridges>, gw:i:<chain_gap_windows>.
 * MDBG_E_IO, MDBG_E_PARAM: as mdbg_gaf_append. */
int mdbg_gaf_append_chains(const char* path, int truncate, const mdbg_chain_list* chains, const mdbg_unitig_list* unitigs, const uint64_t* read_lengths);

#ifdef __cplusplus
}
#endif
#endif
