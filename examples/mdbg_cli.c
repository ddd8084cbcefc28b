/* mdbg_cli.c — the two C ABIs used from plain C, the way rust-mdbg's main() would use them through FFI:
 *   reads.fa[.gz]  ->  mdbg_reader_*  ->  mdbg_ingest_batch[_packed]  ->  mdbg_finalize  ->  mdbg_graph_edges  ->  <prefix>.gfa (+ <prefix>.0.sequences)
 *   --contigs:  ... ->  mdbg_graph_unitigs  ->  mdbg_emit_contigs_*  ->  <prefix>.unitigs.gfa + <prefix>.unitigs.fa   (what the reference's users get from
 *   `gfatools asm -u` + to_basespace + gfa2fasta.sh; no tip or bubble removal)
 *   -c N,L: a small-component step in the schedule (every unitig of a non-circular connected component of at most N nodes and L bases is removed; 0 = no limit
 *   on that side); -e N: an edge-pruning step in the schedule (every edge record crossed by fewer than N resident reads goes where reads leave its source
 *   and enter its target another way: MDBG_SIMPLIFY_EDGES, mdbg_hip.h); -r N: a repeat step (every unitig the resident reads resolve at min_support N is
 *   duplicated, one copy per strong transit key, so the contigs cross it: MDBG_SIMPLIFY_REPEATS; one per schedule, no -e behind it; the copied entries are printed,
 *   and --transits then writes no .msimpl.transits.tsv: no read is placed on a list with copies); -R N: a nested repeat step (MDBG_SIMPLIFY_NESTED: the same at min_support N on a list that may
 *   hold copies, so it may stand behind -r or another -R, any number of times, and resolves a repeat that is one unitig only once its middle has been resolved; no
 *   -e and no -r behind it); -B N,L: a superbubble step (a bubble whose inside branches again, of at most
 *   N entries and L bases inside, 0 = no limit on that side, keeps the path whose weakest unitig is strongest: MDBG_SIMPLIFY_SUPERBUBBLES); --components: the number of connected components of the unitig graph and the largest one (mdbg_graph_components)
 *   --read-paths (implies --contigs): the resident reads threaded through the unitig list (mdbg_graph_read_paths, in ranges of 2^20 reads): one summary line
 *   --junctions (implies --contigs): the reads that cross each edge record of the unitig list (mdbg_graph_junctions, in ranges of 2^20 reads, the supports summed):
 *   one summary line
 *   --transits N (implies --contigs): the reads that span a unitig end to end (mdbg_graph_transits, in ranges of 2^20 reads, the counts merged by key) and whether
 *   the pairs seen N times or more match a repeat's entrances to its exits: <prefix>.unitigs.transits.tsv (and <prefix>.msimpl.transits.tsv) and one summary line each
 *   --gaf (implies --contigs): the resident reads aligned to the unitig list (mdbg_graph_alignments of mdbg_align.h, in ranges of 2^20 reads), one GAF line per
 *   alignment through libmdbg_emit's mdbg_gaf_append: <prefix>.unitigs.gaf (and <prefix>.msimpl.gaf) and one summary line each; qname is the read's ordinal
 *   --query FILE (implies --contigs): the sequences of FILE, which are no part of the graph, aligned to the unitig list without changing it
 *   (mdbg_graph_align_batch): <prefix>.unitigs.query.gaf and <prefix>.unitigs.query.tsv (ordinal, k-min-mers, those found on the list, their share in percent;
 *   and the .msimpl. pair) and one summary line each
 *   --chains S[,G] (implies --contigs): the alignments of a read joined across unplaced windows where the graph bridges them, at max_skew S and max_gap G (0 or
 *   absent: no limit) (mdbg_graph_chains of mdbg_chain.h): <prefix>.unitigs.chains.gaf, one line per chain through mdbg_gaf_append_chains (and
 *   <prefix>.msimpl.chains.gaf); with --query also <prefix>.unitigs.query.chains.gaf and .query.chains.tsv (ordinal, k-min-mers, placed, bridged, the share of
 *   placed + bridged in percent); one summary line each
 *   --keep-reads (with --contigs / --simplify): the context keeps the reads packed on the device (MDBG_FLAG_KEEP_READS) and mdbg_graph_contigs stitches the
 *   sequences there; the same files, and with --no-basespace the input is read once
 *   --sequences-from-kept: the context keeps the reads and the .sequences files are written from that store (mdbg_graph_node_seqs in chunks ->
 *   mdbg_seqfile_write_nodes) instead of in a second pass over the input; the same lines per file, in row order
 * Same flags as the reference binary for this path (src/main.rs:330-420): -k -l --density --minabund --presimp --prefix --threads
 * --reference --skiphpc --syncmers/-s --lmer-counts/--lmer_counts_min/--lmer_counts_max --no-basespace; --contigs is this host's own.
 * --threads N > 1: an uncompressed input is mapped and parsed by N threads (mdbg_reader_open_mt) that also pack their pieces to 2 bits
 * per base (mdbg_reader_next_packed); a reader thread produces batch i+1 while the main thread ingests batch i.
 * Build:  gcc -O2 -Iinclude examples/mdbg_cli.c -Lrust_mdbg_amd -lmdbg_hip -lmdbg_emit -lpthread -Wl,-rpath,$PWD/rust_mdbg_amd -o mdbg_cli
 */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mdbg_align.h"
#include "mdbg_chain.h"
#include "mdbg_emit.h"
#include "mdbg_hip.h"

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

/* reader thread: one batch ahead of the consumer.  The reader alternates two buffer sets (a batch stays valid until the call after
 * the next one), so exactly one batch may be outstanding while the next is parsed and packed. */
typedef struct feed_t {
    mdbg_reader* rd; uint64_t max_bases;
    pthread_mutex_t mu; pthread_cond_t cv;
    int have, rc;                          /* have: a batch is waiting to be picked up */
    mdbg_packed_batch pb;
} feed_t;
static void* feed_main(void* arg) {
    feed_t* f = (feed_t*)arg;
    for (;;) {
        mdbg_packed_batch pb;
        const int rc = mdbg_reader_next_packed(f->rd, f->max_bases, &pb);
        const uint64_t n = rc ? 0 : pb.n_reads;
        pthread_mutex_lock(&f->mu);
        f->pb = pb; f->rc = rc; f->have = 1;
        pthread_cond_broadcast(&f->cv);
        while (f->have) pthread_cond_wait(&f->cv, &f->mu);          /* picking batch j up means the consumer is done with batch j-1: its buffer may be reused */
        pthread_mutex_unlock(&f->mu);
        if (rc || !n) return NULL;
    }
}
/* next batch from the reader thread (the previous one must have been fully consumed) */
static int feed_take(feed_t* f, mdbg_packed_batch* pb) {
    pthread_mutex_lock(&f->mu);
    while (!f->have) pthread_cond_wait(&f->cv, &f->mu);
    *pb = f->pb;
    const int rc = f->rc;
    f->have = 0;
    pthread_cond_broadcast(&f->cv);
    pthread_mutex_unlock(&f->mu);
    return rc;
}

/* one writer of the .sequences pass: the lines of the nodes i with i % n_parts == part of the current batch, into its own file */
typedef struct seqjob_t { mdbg_seqfile* sf; const mdbg_nodes* nodes; uint32_t part, n_parts; const uint8_t* bases; const uint64_t* offs; uint64_t n, first; int rc; } seqjob_t;
static void* seqjob_main(void* arg) {
    seqjob_t* j = (seqjob_t*)arg;
    j->rc = mdbg_seqfile_write_batch_part(j->sf, j->nodes, j->part, j->n_parts, j->bases, j->offs, j->n, j->first);
    return NULL;
}

/* one writer of the kept-reads path: the lines of the rows i with i % n_parts == part of the current chunk of node sequences */
typedef struct nodejob_t { mdbg_seqfile* sf; const mdbg_nodes* nodes; uint32_t part, n_parts; const mdbg_node_seqs* chunk; int rc; } nodejob_t;
static void* nodejob_main(void* arg) {
    nodejob_t* j = (nodejob_t*)arg;
    j->rc = mdbg_seqfile_write_nodes(j->sf, j->nodes, j->part, j->n_parts, j->chunk->first_row, j->chunk->n_rows, j->chunk->bases, j->chunk->offsets);
    return NULL;
}

static void die(mdbg_ctx* ctx, const char* what, int rc) {
    fprintf(stderr, "%s: %s (%s)\n", what, mdbg_strerror(rc), ctx && mdbg_last_error(ctx) ? mdbg_last_error(ctx) : "");
    exit(1);
}

/* ---- --gaf and --query: alignments (mdbg_align.h) as GAF lines, through libmdbg_emit's writer ---- */
static uint64_t* note_lengths(uint64_t* lens, uint64_t* cap, uint64_t first, const uint64_t* offs, uint64_t n) {
    if (first + n > *cap) {
        *cap = 2 * (first + n) + 1024;
        lens = (uint64_t*)realloc(lens, *cap * sizeof *lens);
        if (!lens) die(NULL, "realloc", MDBG_E_NOMEM);
    }
    for (uint64_t q = 0; q < n; ++q) lens[first + q] = offs[q + 1] - offs[q];
    return lens;
}
/* the resident reads in ranges of 2^20, the writer appending range after range; lens[q] = the raw length of read q */
static void write_gaf(mdbg_ctx* ctx, const mdbg_unitig_list* ul, const char* path, const uint64_t* lens, const char* what) {
    uint64_t first = 0, n_aln = 0, n_chained = 0;
    FILE* f = fopen(path, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    fclose(f);
    for (;;) {
        mdbg_alignment_list al;
        int rc = mdbg_graph_alignments(ctx, first, (uint64_t)1 << 20, &al);
        if (rc) die(ctx, "mdbg_graph_alignments", rc);
        if (!al.n_reads) break;
        rc = mdbg_gaf_append(path, 0, &al, ul, lens + first);
        if (rc) die(NULL, "mdbg_gaf_append", rc);
        n_aln += al.n_alignments; n_chained += al.n_chained; first += al.n_reads;
    }
    printf("alignments%s: %llu of %llu reads, %llu steps chained over a record\n", what, (unsigned long long)n_aln, (unsigned long long)first, (unsigned long long)n_chained);
}
/* the sequences of `file`, which are no part of the graph, in the reader's batches: <stem>.query.gaf and <stem>.query.tsv (ordinal, windows, placed, percent) */
static void write_query(mdbg_ctx* ctx, const mdbg_unitig_list* ul, const char* stem, const char* file, int reference, const char* what) {
    char gaf[4096], tsv[4096];
    int err = 0;
    uint64_t first = 0, n_aln = 0, n_found = 0;
    snprintf(gaf, sizeof gaf, "%s.query.gaf", stem); snprintf(tsv, sizeof tsv, "%s.query.tsv", stem);
    FILE* f = fopen(gaf, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    fclose(f);
    f = fopen(tsv, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    mdbg_reader* rd = mdbg_reader_open(file, reference, &err);
    if (!rd) die(NULL, "mdbg_reader_open", err);
    for (;;) {
        const uint8_t* bases; const uint64_t* offs; uint64_t n;
        int rc = mdbg_reader_next(rd, 256u << 20, &bases, &offs, &n);
        if (rc) die(NULL, "mdbg_reader_next", rc);
        if (!n) break;
        mdbg_alignment_list al;
        rc = mdbg_graph_align_batch(ctx, bases, offs, n, &al);
        if (rc) die(ctx, "mdbg_graph_align_batch", rc);
        uint64_t* lens = (uint64_t*)malloc(2 * n * sizeof *lens);    /* the lengths, and the ordinals in the FILE: the call numbers a batch from 0 */
        if (!lens) die(NULL, "malloc", MDBG_E_NOMEM);
        uint64_t* ord = lens + n;
        for (uint64_t q = 0; q < n; ++q) { lens[q] = offs[q + 1] - offs[q]; ord[q] = first + q; }
        al.ordinal = ord;
        rc = mdbg_gaf_append(gaf, 0, &al, ul, lens);
        if (rc) die(NULL, "mdbg_gaf_append", rc);
        for (uint64_t q = 0; q < al.n_reads; ++q) {
            uint64_t placed = 0;
            for (uint64_t s = al.step_offsets[q]; s < al.step_offsets[q + 1]; ++s) placed += al.step_windows[s];
            const uint32_t w = al.read_windows[q];
            fprintf(f, "%llu\t%u\t%llu\t%.2f\n", (unsigned long long)ord[q], w, (unsigned long long)placed, w ? 100.0 * (double)placed / (double)w : 0.0);
            n_found += placed > 0;
        }
        free(lens);
        n_aln += al.n_alignments; first += n;
    }
    mdbg_reader_close(rd);
    if (fclose(f) != 0) die(NULL, "fclose", MDBG_E_IO);
    printf("query%s: %llu sequences, %llu with a k-min-mer on the list, %llu alignments\n", what, (unsigned long long)first, (unsigned long long)n_found, (unsigned long long)n_aln);
}

/* ---- --chains: the same two writers over mdbg_graph_chains / mdbg_graph_chain_batch (mdbg_chain.h) ---- */
static void write_chains(mdbg_ctx* ctx, const mdbg_unitig_list* ul, const char* path, const uint64_t* lens, uint32_t skew, uint32_t gap, const char* what) {
    uint64_t first = 0, n_chains = 0, n_inside = 0, n_record = 0, n_gapw = 0;
    FILE* f = fopen(path, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    fclose(f);
    for (;;) {
        mdbg_chain_list ch;
        int rc = mdbg_graph_chains(ctx, first, (uint64_t)1 << 20, skew, gap, &ch);
        if (rc) die(ctx, "mdbg_graph_chains", rc);
        if (!ch.alignments.n_reads) break;
        rc = mdbg_gaf_append_chains(path, 0, &ch, ul, lens + first);
        if (rc) die(NULL, "mdbg_gaf_append_chains", rc);
        n_chains += ch.n_chains; n_inside += ch.n_bridges_inside; n_record += ch.n_bridges_record; n_gapw += ch.n_gap_windows; first += ch.alignments.n_reads;
    }
    printf("chains%s: %llu reads, %llu chains, %llu bridges inside a unitig, %llu over a record, %llu windows in bridged gaps\n", what, (unsigned long long)first,
           (unsigned long long)n_chains, (unsigned long long)n_inside, (unsigned long long)n_record, (unsigned long long)n_gapw);
}
static void write_query_chains(mdbg_ctx* ctx, const mdbg_unitig_list* ul, const char* stem, const char* file, int reference, uint32_t skew, uint32_t gap, const char* what) {
    char gaf[4096], tsv[4096];
    int err = 0;
    uint64_t first = 0, n_chains = 0, n_bridges = 0;
    snprintf(gaf, sizeof gaf, "%s.query.chains.gaf", stem); snprintf(tsv, sizeof tsv, "%s.query.chains.tsv", stem);
    FILE* f = fopen(gaf, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    fclose(f);
    f = fopen(tsv, "wb");
    if (!f) die(NULL, "fopen", MDBG_E_IO);
    mdbg_reader* rd = mdbg_reader_open(file, reference, &err);
    if (!rd) die(NULL, "mdbg_reader_open", err);
    for (;;) {
        const uint8_t* bases; const uint64_t* offs; uint64_t n;
        int rc = mdbg_reader_next(rd, 256u << 20, &bases, &offs, &n);
        if (rc) die(NULL, "mdbg_reader_next", rc);
        if (!n) break;
        mdbg_chain_list ch;
        rc = mdbg_graph_chain_batch(ctx, bases, offs, n, skew, gap, &ch);
        if (rc) die(ctx, "mdbg_graph_chain_batch", rc);
        uint64_t* lens = (uint64_t*)malloc(2 * n * sizeof *lens);    /* the lengths, and the ordinals in the FILE: the call numbers a batch from 0 */
        if (!lens) die(NULL, "malloc", MDBG_E_NOMEM);
        uint64_t* ord = lens + n;
        for (uint64_t q = 0; q < n; ++q) { lens[q] = offs[q + 1] - offs[q]; ord[q] = first + q; }
        ch.alignments.ordinal = ord;
        rc = mdbg_gaf_append_chains(gaf, 0, &ch, ul, lens);
        if (rc) die(NULL, "mdbg_gaf_append_chains", rc);
        for (uint64_t q = 0; q < ch.alignments.n_reads; ++q) {
            uint64_t placed = 0, bridged = 0;
            for (uint64_t c = ch.chain_offsets[q]; c < ch.chain_offsets[q + 1]; ++c) { placed += ch.chain_windows[c]; bridged += ch.chain_gap_windows[c]; }
            const uint32_t w = ch.alignments.read_windows[q];
            fprintf(f, "%llu\t%u\t%llu\t%llu\t%.2f\n", (unsigned long long)ord[q], w, (unsigned long long)placed, (unsigned long long)bridged,
                    w ? 100.0 * (double)(placed + bridged) / (double)w : 0.0);
        }
        free(lens);
        n_chains += ch.n_chains; n_bridges += ch.n_bridges; first += n;
    }
    mdbg_reader_close(rd);
    if (fclose(f) != 0) die(NULL, "fclose", MDBG_E_IO);
    printf("query chains%s: %llu sequences, %llu chains, %llu bridges\n", what, (unsigned long long)first, (unsigned long long)n_chains, (unsigned long long)n_bridges);
}

/* ---- --transits: the rows of the ranges merged by key, the verdict rule of mdbg_graph_transits on the merged counts, the .transits.tsv ---- */
typedef struct trow_t { uint32_t u, pu, pj, ps, qu, qj, qs; uint64_t count; } trow_t;
static int trow_cmp(const void* a, const void* b) {
    const trow_t* x = (const trow_t*)a; const trow_t* y = (const trow_t*)b;
    const uint32_t kx[7] = {x->u, x->pu, x->pj, x->ps, x->qu, x->qj, x->qs}, ky[7] = {y->u, y->pu, y->pj, y->ps, y->qu, y->qj, y->qs};
    for (int i = 0; i < 7; ++i) if (kx[i] != ky[i]) return kx[i] < ky[i] ? -1 : 1;
    return 0;
}
static int u64_cmp(const void* a, const void* b) { const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b; return x < y ? -1 : x > y; }
static void* must(void* p) { if (!p) { fprintf(stderr, "out of memory\n"); exit(1); } return p; }
static void write_transits(mdbg_ctx* ctx, const mdbg_unitig_list* ul, const char* path, uint64_t min_support, const char* label) {
    static const char* const verdict_name[4] = {"plain", "resolved", "unresolved", "self"};
    trow_t* rows = NULL; uint64_t n = 0, cap = 0, first = 0, U = 0, n_passes = 0, n_repeats = 0, n_resolved = 0;
    uint32_t* n_in = NULL; uint32_t* n_out = NULL; uint64_t* passes = NULL;
    for (;;) {
        mdbg_transit_list t;
        const int rc = mdbg_graph_transits(ctx, first, (uint64_t)1 << 20, min_support, &t);
        if (rc) die(ctx, "mdbg_graph_transits", rc);
        if (!t.n_reads) break;
        if (!passes) {                                              /* n_in and n_out depend on the records alone: any range's */
            U = t.n_unitigs;
            n_in = (uint32_t*)must(malloc(U * sizeof *n_in)); n_out = (uint32_t*)must(malloc(U * sizeof *n_out)); passes = (uint64_t*)must(calloc(U, sizeof *passes));
            memcpy(n_in, t.n_in, U * sizeof *n_in); memcpy(n_out, t.n_out, U * sizeof *n_out);
        }
        for (uint64_t u = 0; u < U; ++u) passes[u] += t.passes[u];
        if (n + t.n_transits > cap) { cap = 2 * (n + t.n_transits); rows = (trow_t*)must(realloc(rows, cap * sizeof *rows)); }
        for (uint64_t i = 0; i < t.n_transits; ++i) {
            trow_t r; r.u = t.unitig[i]; r.pu = t.in_unitig[i]; r.pj = t.in_entry[i]; r.ps = t.in_strand[i]; r.qu = t.out_unitig[i]; r.qj = t.out_entry[i]; r.qs = t.out_strand[i];
            r.count = t.count[i];
            rows[n++] = r;
        }
        n_passes += t.n_passes; first += t.n_reads;
    }
    if (n) qsort(rows, n, sizeof *rows, trow_cmp);
    uint64_t m = 0;                                                 /* equal keys of different ranges fall together */
    for (uint64_t i = 0; i < n; ++i) if (m && !trow_cmp(&rows[m - 1], &rows[i])) rows[m - 1].count += rows[i].count; else rows[m++] = rows[i];
    uint8_t* self = (uint8_t*)must(calloc(U + 1, 1));
    for (uint64_t r = 0; r < ul->edges.n && U; ++r) if (ul->edges.n1[r] == ul->edges.n2[r]) self[ul->edges.n1[r]] = 1;
    uint64_t* qs = (uint64_t*)must(malloc((m + 1) * sizeof *qs));
    FILE* f = fopen(path, "w");
    if (!f) { perror(path); exit(1); }
    for (uint64_t i = 0; i < m; ++i)
        fprintf(f, "T\tutg%07u%c\t%c\tutg%07u%c\t+\tutg%07u%c\t%c\t%llu\n", rows[i].pu + 1, ul->circular[rows[i].pu] ? 'c' : 'l', rows[i].ps ? '-' : '+', rows[i].u + 1,
                ul->circular[rows[i].u] ? 'c' : 'l', rows[i].qu + 1, ul->circular[rows[i].qu] ? 'c' : 'l', rows[i].qs ? '-' : '+', (unsigned long long)rows[i].count);
    uint64_t at = 0;
    for (uint64_t u = 0; u < U; ++u) {
        uint64_t strong = 0; int matched = 1; const trow_t* last = NULL;
        for (; at < m && rows[at].u == u; ++at) {
            if (rows[at].count < min_support) continue;
            if (last && last->pu == rows[at].pu && last->pj == rows[at].pj && last->ps == rows[at].ps) matched = 0;      /* (equal p are neighbours in key order) */
            last = &rows[at];
            qs[strong++] = (uint64_t)rows[at].qu << 33 | (uint64_t)rows[at].qj << 1 | rows[at].qs;
        }
        if (n_in[u] < 2 || n_out[u] < 2) continue;
        qsort(qs, strong, sizeof *qs, u64_cmp);
        for (uint64_t i = 1; i < strong; ++i) if (qs[i] == qs[i - 1]) matched = 0;
        const int v = self[u] ? MDBG_TRANSIT_SELF : n_in[u] == n_out[u] && strong == n_in[u] && matched ? MDBG_TRANSIT_RESOLVED : MDBG_TRANSIT_UNRESOLVED;
        ++n_repeats; n_resolved += v == MDBG_TRANSIT_RESOLVED;
        fprintf(f, "U\tutg%07llu%c\t%u\t%u\t%llu\t%s\n", (unsigned long long)u + 1, ul->circular[u] ? 'c' : 'l', n_in[u], n_out[u], (unsigned long long)passes[u], verdict_name[v]);
    }
    if (fclose(f)) { perror(path); exit(1); }
    printf("transits%s: %llu keys, %llu passes, %llu repeats, %llu of them resolved at min_support %llu\n", label, (unsigned long long)m, (unsigned long long)n_passes,
           (unsigned long long)n_repeats, (unsigned long long)n_resolved, (unsigned long long)min_support);
    free(rows); free(n_in); free(n_out); free(passes); free(self); free(qs);
}

int main(int argc, char** argv) {
    mdbg_params p; memset(&p, 0, sizeof p);
    p.k = 10; p.l = 12; p.density = 0.1; p.min_abundance = 2; p.device = -1;       /* the reference's defaults (main.rs:430-450) */
    float presimp = 0.01f;
    const char* input = NULL; const char* prefix = "graph"; int write_sequences = 1, threads = 1, reference = 0, timing = 0, contigs = 0, keep_reads = 0, seq_kept = 0, components = 0, read_paths = 0, junctions = 0, gaf = 0, chains = 0; uint64_t transits = 0; const char* query = NULL; unsigned chain_skew = 0, chain_gap = 0;
    const char* lmer_counts = NULL; uint32_t lc_min = 2, lc_max = 100000;          /* main.rs:447-448 */
    int syncmer_s_given = 0;
    /* the first `gfatools asm` line of utils/magic_simplify as steps (--simplify); -t N,L / -b L / -c N,L / -e N / -r N / -R N / -B N,L append steps of their own, in command-line order */
    static const mdbg_simplify_step magic[] = {{MDBG_SIMPLIFY_TIPS, 10, 50000}, {MDBG_SIMPLIFY_TIPS, 10, 50000}, {MDBG_SIMPLIFY_BUBBLES, 0, 100000}, {MDBG_SIMPLIFY_BUBBLES, 0, 100000},
        {MDBG_SIMPLIFY_TIPS, 10, 50000}, {MDBG_SIMPLIFY_BUBBLES, 0, 100000}, {MDBG_SIMPLIFY_BUBBLES, 0, 100000}, {MDBG_SIMPLIFY_BUBBLES, 0, 100000}, {MDBG_SIMPLIFY_TIPS, 10, 50000},
        {MDBG_SIMPLIFY_BUBBLES, 0, 100000}, {MDBG_SIMPLIFY_TIPS, 10, 50000}, {MDBG_SIMPLIFY_BUBBLES, 0, 1000000}, {MDBG_SIMPLIFY_TIPS, 10, 150000}, {MDBG_SIMPLIFY_BUBBLES, 0, 1000000}};
    enum { MAX_STEPS = 256 };
    mdbg_simplify_step steps[MAX_STEPS]; uint32_t n_steps = 0; int simplify = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-k") && i + 1 < argc) p.k = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-l") && i + 1 < argc) p.l = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--density") && i + 1 < argc) p.density = atof(argv[++i]);
        else if (!strcmp(argv[i], "--minabund") && i + 1 < argc) p.min_abundance = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--presimp") && i + 1 < argc) presimp = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if (!strcmp(argv[i], "--no-basespace")) write_sequences = 0;
        else if (!strcmp(argv[i], "--threads") && i + 1 < argc) threads = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--reference")) reference = 1;                                 /* main.rs:737: newlines inside FASTA records are removed */
        else if (!strcmp(argv[i], "--lmer-counts") && i + 1 < argc) lmer_counts = argv[++i];
        else if (!strcmp(argv[i], "--lmer_counts_min") && i + 1 < argc) lc_min = (uint32_t)strtoul(argv[++i], NULL, 10);
        else if (!strcmp(argv[i], "--lmer_counts_max") && i + 1 < argc) lc_max = (uint32_t)strtoul(argv[++i], NULL, 10);
        else if (!strcmp(argv[i], "--timing")) timing = 1;
        else if (!strcmp(argv[i], "--contigs")) contigs = 1;
        else if (!strcmp(argv[i], "--keep-reads")) keep_reads = 1;
        else if (!strcmp(argv[i], "--sequences-from-kept")) seq_kept = 1;
        else if (!strcmp(argv[i], "--simplify")) {
            simplify = 1;
            for (uint32_t j = 0; j < sizeof magic / sizeof magic[0] && n_steps < MAX_STEPS; ++j) steps[n_steps++] = magic[j];
        }
        else if ((!strcmp(argv[i], "-t") || !strcmp(argv[i], "-b")) && i + 1 < argc) {
            const int tip = argv[i][1] == 't';
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = tip ? MDBG_SIMPLIFY_TIPS : MDBG_SIMPLIFY_BUBBLES; st.max_nodes = 0;
            if (tip) { st.max_nodes = (uint32_t)strtoul(a, &end, 10); if (*end != ',') { fprintf(stderr, "-t wants N,L\n"); return 2; } a = end + 1; }
            st.max_bases = strtoull(a, &end, 10);
            if (*end || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "-c") && i + 1 < argc) {
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = MDBG_SIMPLIFY_COMPONENTS;
            st.max_nodes = (uint32_t)strtoul(a, &end, 10);
            if (*end != ',') { fprintf(stderr, "-c wants N,L\n"); return 2; }
            st.max_bases = strtoull(end + 1, &end, 10);
            if (*end || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b / -c\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "-e") && i + 1 < argc) {
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = MDBG_SIMPLIFY_EDGES; st.max_bases = 0;
            st.max_nodes = (uint32_t)strtoul(a, &end, 10);              /* (the field carries min_support for this kind) */
            if (*end || !*a || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b / -c / -e\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) {              /* the unitigs the reads resolve at min_support N are duplicated (one per schedule, no -e behind it) */
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = MDBG_SIMPLIFY_REPEATS; st.max_bases = 0;
            st.max_nodes = (uint32_t)strtoul(a, &end, 10);              /* (the field carries min_support for this kind) */
            if (*end || !*a || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b / -c / -e / -r / -R\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "-R") && i + 1 < argc) {              /* a repeat step on a list that may hold copies: behind -r or another -R (no -e, no -r behind it) */
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = MDBG_SIMPLIFY_NESTED; st.max_bases = 0;
            st.max_nodes = (uint32_t)strtoul(a, &end, 10);              /* (the field carries min_support for this kind) */
            if (*end || !*a || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b / -c / -e / -r / -R\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "-B") && i + 1 < argc) {              /* bubbles whose inside branches: a bubble of at most N entries and L bases inside keeps its strongest path */
            char* end = NULL; const char* a = argv[++i];
            mdbg_simplify_step st; st.kind = MDBG_SIMPLIFY_SUPERBUBBLES;
            st.max_nodes = (uint32_t)strtoul(a, &end, 10);
            if (*end != ',') { fprintf(stderr, "-B wants N,L\n"); return 2; }
            st.max_bases = strtoull(end + 1, &end, 10);
            if (*end || n_steps >= MAX_STEPS) { fprintf(stderr, "bad or too many -t / -b / -c / -e / -r / -B\n"); return 2; }
            steps[n_steps++] = st; simplify = 1;
        }
        else if (!strcmp(argv[i], "--components")) components = 1;
        else if (!strcmp(argv[i], "--read-paths")) read_paths = 1;
        else if (!strcmp(argv[i], "--junctions")) junctions = 1;
        else if (!strcmp(argv[i], "--transits") && i + 1 < argc) { transits = strtoull(argv[++i], NULL, 10); if (!transits) { fprintf(stderr, "--transits takes a min_support >= 1\n"); return 2; } }
        else if (!strcmp(argv[i], "--gaf")) gaf = 1;
        else if (!strcmp(argv[i], "--chains") && i + 1 < argc) { chains = 1; chain_gap = 0; if (sscanf(argv[++i], "%u,%u", &chain_skew, &chain_gap) < 1) { fprintf(stderr, "--chains S[,G]\n"); return 2; } }
        else if (!strcmp(argv[i], "--query") && i + 1 < argc) query = argv[++i];
        else if (!strcmp(argv[i], "--bf")) p.flags |= MDBG_FLAG_PREFILTER;                      /* main.rs --bf, order-free: the counting pre-filter in front of the node table */
        else if (!strcmp(argv[i], "--bf-cells") && i + 1 < argc) p.prefilter_cells = strtoull(argv[++i], NULL, 10);   /* its number of 2-bit cells (default 2^32) */
        else if (!strcmp(argv[i], "--skiphpc")) p.reads_already_hpc = 1;                         /* main.rs:490 */
        else if (!strcmp(argv[i], "--syncmers")) { p.scheme = MDBG_SCHEME_SYNCMERS; if (!syncmer_s_given) p.syncmer_s = 4; }       /* main.rs:438,491-495: default s = 4 */
        else if ((!strcmp(argv[i], "-s") || !strcmp(argv[i], "--s")) && i + 1 < argc) { p.syncmer_s = (uint32_t)atoi(argv[++i]); syncmer_s_given = 1; }
        else if (argv[i][0] != '-') input = argv[i];
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (!input) { fprintf(stderr, "usage: mdbg_cli reads.fa[.gz] [-k K] [-l L] [--density D] [--minabund A] [--presimp P] [--prefix PFX] [--no-basespace] [--threads N] [--reference] [--skiphpc] [--bf [--bf-cells N]] [--syncmers [-s S]] [--lmer-counts FILE [--lmer_counts_min A] [--lmer_counts_max B]] [--contigs] [--simplify] [-t N,L] [-b L] [-c N,L] [-e N] [-r N] [-R N] [-B N,L] [--components] [--read-paths] [--junctions] [--transits N] [--gaf] [--chains S[,G]] [--query FILE] [--keep-reads] [--sequences-from-kept] [--timing]\n"); return 2; }
    if (threads < 1) threads = 1;
    if (simplify || components || read_paths || junctions || transits || gaf || chains || query) contigs = 1;
    if (!contigs) keep_reads = 0;
    if (!write_sequences) seq_kept = 0;
    if (keep_reads || seq_kept) p.flags |= MDBG_FLAG_KEEP_READS;      /* (--sequences-from-kept keeps the reads by itself; the contigs come from the store only with --keep-reads) */

    int err = 0;
    mdbg_ctx* ctx = mdbg_create(&p, &err);
    if (!ctx) die(NULL, "mdbg_create", err);
    const double t0 = now_s();
    if (lmer_counts) {                                               /* main.rs:544-575: the selected l-mers restrict the sketch */
        uint64_t* codes = NULL; uint64_t n_codes = 0, ignored = 0;
        int rc = mdbg_lmer_filter_from_counts(lmer_counts, p.l, p.density, lc_min, lc_max, &codes, &n_codes, &ignored);
        if (rc) die(NULL, "mdbg_lmer_filter_from_counts", rc);
        rc = mdbg_set_lmer_filter(ctx, codes, n_codes);
        if (rc) die(ctx, "mdbg_set_lmer_filter", rc);
        mdbg_lmer_filter_free(codes);
    }
    const uint64_t batch_bases = 256u << 20;
    mdbg_reader* rd = mdbg_reader_open_mt(input, reference, threads, &err);
    if (!rd) die(NULL, "mdbg_reader_open", err);
    /* the batch buffers come from the GPU library: page-locked by the first ingest call that sees them, so a batch crosses PCIe as one DMA */
    { const int rc = mdbg_reader_set_allocator(rd, mdbg_host_alloc, mdbg_host_free); if (rc) die(NULL, "mdbg_reader_set_allocator", rc); }
    uint64_t n_reads = 0, n_bases = 0, first = 0;
    uint64_t* read_lens = NULL; uint64_t lens_cap = 0;              /* --gaf: the raw length of every read, from the batch offsets */
    double t_wait = 0, t_gpu = 0;                                   /* --timing: where the ingest loop spends its time */
    if (threads > 1) {                                              /* any input: the streaming reader (.gz, .lz4) packs on the reader thread */
        /* reader thread one batch ahead; this thread packs to 2 bits per base and ingests */
        feed_t f; memset(&f, 0, sizeof f); f.rd = rd; f.max_bases = batch_bases;
        pthread_mutex_init(&f.mu, NULL); pthread_cond_init(&f.cv, NULL);
        pthread_t th; pthread_create(&th, NULL, feed_main, &f);
        for (;;) {
            mdbg_packed_batch pb;
            double ta = now_s();
            int rc = feed_take(&f, &pb);
            t_wait += now_s() - ta;
            if (rc) die(NULL, "mdbg_reader_next_packed", rc);
            if (!pb.n_reads) break;
            ta = now_s();
            rc = mdbg_ingest_batch_packed(ctx, &pb, first);
            if (rc) die(ctx, "mdbg_ingest_batch_packed", rc);
            t_gpu += now_s() - ta;
            if (gaf || chains) read_lens = note_lengths(read_lens, &lens_cap, first, pb.offsets, pb.n_reads);
            first += pb.n_reads; n_reads += pb.n_reads; n_bases += pb.offsets[pb.n_reads];
        }
        pthread_join(th, NULL);
    } else for (;;) {
        const uint8_t* bases; const uint64_t* offs; uint64_t n;
        int rc = mdbg_reader_next(rd, batch_bases, &bases, &offs, &n);
        if (rc) die(NULL, "mdbg_reader_next", rc);
        if (!n) break;
        rc = mdbg_ingest_batch(ctx, bases, offs, n, first);          /* process_read_aux over the batch */
        if (rc) die(ctx, "mdbg_ingest_batch", rc);
        if (gaf || chains) read_lens = note_lengths(read_lens, &lens_cap, first, offs, n);
        first += n; n_reads += n; n_bases += offs[n];
    }
    mdbg_reader_close(rd);
    const double t_ingest = now_s();

    mdbg_nodes nodes; mdbg_edge_list edges;
    /* without the .sequences pass the host prints three columns of the node table (the S lines): the minimizer lists stay on the device */
    int rc = write_sequences ? mdbg_finalize(ctx, &nodes) : mdbg_finalize_gfa(ctx, &nodes);
    if (rc) die(ctx, "mdbg_finalize", rc);
    rc = mdbg_graph_edges(ctx, presimp, &edges);
    if (rc) die(ctx, "mdbg_graph_edges", rc);
    if (p.min_abundance > 1) {                                      /* what the reference prints (main.rs:926-928, 1118-1120) */
        printf("Number of nodes before abundance filter: %llu\n", (unsigned long long)nodes.n_distinct);
        printf("Number of nodes after abundance filter: %llu\n", (unsigned long long)nodes.n);
    } else printf("Number of mdBG nodes: %llu\n", (unsigned long long)nodes.n);
    printf("Number of mdBG edges: %llu\n", (unsigned long long)edges.n);
    printf("Pre-simp = %g: %llu edges removed\n", presimp, (unsigned long long)edges.presimp_removed);

    char path[4096];
    snprintf(path, sizeof path, "%s.gfa", prefix);
    rc = mdbg_emit_write_gfa(path, &nodes, &edges);
    if (rc) die(NULL, "mdbg_emit_write_gfa", rc);
    if (timing) fprintf(stderr, "timing: %llu reads, %llu bases; ingest %.3f s, to .gfa %.3f s (%.2f Gbases/s; context creation not included); ingest loop: waiting for the reader %.3f, mdbg_ingest_batch_packed %.3f s\n",
                        (unsigned long long)n_reads, (unsigned long long)n_bases, t_ingest - t0, now_s() - t0, (double)n_bases / (now_s() - t0) / 1e9, t_wait, t_gpu);
    if (seq_kept) {                                                 /* the node sequences from the device store, chunk by chunk, while the node table is current */
        enum { MAX_KEPT_WRITERS = 16 };
        const int nw = threads > MAX_KEPT_WRITERS ? MAX_KEPT_WRITERS : threads;
        mdbg_seqfile* sf[MAX_KEPT_WRITERS]; nodejob_t job[MAX_KEPT_WRITERS]; pthread_t th[MAX_KEPT_WRITERS];
        const double ts = now_s();
        double ms_gather = 0; uint64_t n_chunks = 0, n_seq_bases = 0;
        for (int t = 0; t < nw; ++t) {
            snprintf(path, sizeof path, "%s.%d.sequences", prefix, t);
            sf[t] = mdbg_seqfile_open(path, p.k, p.l, &err);
            if (!sf[t]) die(NULL, "mdbg_seqfile_open", err);
        }
        for (uint64_t row = 0;;) {
            mdbg_node_seqs ch; double ms = 0;
            rc = mdbg_graph_node_seqs(ctx, row, 0, 256u << 20, &ch);
            if (rc) die(ctx, "mdbg_graph_node_seqs", rc);
            if (!ch.n_rows) break;
            mdbg_node_seqs_ms(ctx, &ms); ms_gather += ms; ++n_chunks; n_seq_bases += ch.n_bases;
            for (int t = 0; t < nw; ++t) {
                nodejob_t jb; jb.sf = sf[t]; jb.nodes = &nodes; jb.part = (uint32_t)t; jb.n_parts = (uint32_t)nw; jb.chunk = &ch; jb.rc = 0;
                job[t] = jb;
                if (t) pthread_create(&th[t], NULL, nodejob_main, &job[t]);
            }
            nodejob_main(&job[0]);
            for (int t = 1; t < nw; ++t) pthread_join(th[t], NULL);
            for (int t = 0; t < nw; ++t) if (job[t].rc) die(NULL, "mdbg_seqfile_write_nodes", job[t].rc);
            row += ch.n_rows;
        }
        for (int t = 0; t < nw; ++t) { rc = mdbg_seqfile_close(sf[t]); if (rc) die(NULL, "mdbg_seqfile_close", rc); }
        if (timing) fprintf(stderr, "timing: .sequences from the kept reads %.3f s (%d file%s; %llu chunks, %llu bases, gather kernel %.3f ms)\n", now_s() - ts, nw, nw > 1 ? "s" : "",
                            (unsigned long long)n_chunks, (unsigned long long)n_seq_bases, ms_gather);
    }
    mdbg_contigs* ctg = NULL; mdbg_contigs* sctg = NULL;
    if (simplify) {                                                 /* tips and simple bubbles removed on the GPU (this project's own rules, not gfatools parity: mdbg_hip.h) */
        mdbg_unitig_list sl; mdbg_simplify_stats ss;
        rc = mdbg_graph_simplify(ctx, steps, n_steps, &sl, &ss);
        if (rc) die(ctx, "mdbg_graph_simplify", rc);
        const uint64_t* edges_removed = NULL; uint64_t total_edges_removed = 0; int edge_steps = 0, repeat_steps = 0;
        rc = mdbg_simplify_edges_removed(ctx, &edges_removed, &total_edges_removed);
        if (rc) die(ctx, "mdbg_simplify_edges_removed", rc);
        for (uint32_t j = 0; j < ss.n_steps; ++j)
            if (steps[j].kind == MDBG_SIMPLIFY_REPEATS || steps[j].kind == MDBG_SIMPLIFY_NESTED) { printf("simplify step %u (%s %u)\n", j + 1, steps[j].kind == MDBG_SIMPLIFY_NESTED ? "nested repeats" : "repeats", steps[j].max_nodes); repeat_steps = 1; }
            else if (steps[j].kind == MDBG_SIMPLIFY_EDGES) { printf("simplify step %u (edges %u): %llu edge records removed\n", j + 1, steps[j].max_nodes, (unsigned long long)edges_removed[j]); edge_steps = 1; }
            else printf("simplify step %u (%s %u,%llu): %llu unitigs, %llu nodes removed\n", j + 1, steps[j].kind == MDBG_SIMPLIFY_TIPS ? "tips" : steps[j].kind == MDBG_SIMPLIFY_BUBBLES ? "bubbles" : steps[j].kind == MDBG_SIMPLIFY_SUPERBUBBLES ? "superbubbles" : "components", steps[j].max_nodes,
                   (unsigned long long)steps[j].max_bases, (unsigned long long)ss.unitigs_removed[j], (unsigned long long)ss.nodes_removed[j]);
        printf("simplify: %llu unitigs, %llu nodes removed; %llu contigs left\n", (unsigned long long)ss.total_unitigs_removed, (unsigned long long)ss.total_nodes_removed,
               (unsigned long long)sl.n_unitigs);
        if (edge_steps) printf("simplify: %llu edge records removed\n", (unsigned long long)total_edges_removed);
        /* n_entries == rows of the node table - total_nodes_removed + copies (mdbg_hip.h); no read is placed on a list with copies: no .msimpl.transits.tsv then */
        if (repeat_steps) printf("simplify: %llu entries copied\n", (unsigned long long)(sl.n_entries ? sl.n_entries + ss.total_nodes_removed - nodes.n : 0));
        if (transits && !repeat_steps) { snprintf(path, sizeof path, "%s.msimpl.transits.tsv", prefix); write_transits(ctx, &sl, path, transits, " (simplified)"); }
        if (gaf && !repeat_steps) { snprintf(path, sizeof path, "%s.msimpl.gaf", prefix); write_gaf(ctx, &sl, path, read_lens, " (simplified)"); }
        if (query && !repeat_steps) { snprintf(path, sizeof path, "%s.msimpl", prefix); write_query(ctx, &sl, path, query, reference, " (simplified)"); }
        if (chains && !repeat_steps) {
            snprintf(path, sizeof path, "%s.msimpl.chains.gaf", prefix); write_chains(ctx, &sl, path, read_lens, chain_skew, chain_gap, " (simplified)");
            if (query) { snprintf(path, sizeof path, "%s.msimpl", prefix); write_query_chains(ctx, &sl, path, query, reference, chain_skew, chain_gap, " (simplified)"); }
        }
        sctg = mdbg_emit_contigs_open(&sl, NULL, &err);             /* (no node table: the list covers the surviving nodes only) */
        if (!sctg) die(NULL, "mdbg_emit_contigs_open", err);
        if (keep_reads) {                                           /* the sequences from the device store instead of the second pass */
            mdbg_contig_seqs cs;
            rc = mdbg_graph_contigs(ctx, 0, &cs);
            if (rc) die(ctx, "mdbg_graph_contigs", rc);
            rc = mdbg_emit_contigs_set_sequences(sctg, cs.bases, cs.offsets, cs.n_contigs);
            if (rc) die(NULL, "mdbg_emit_contigs_set_sequences", rc);
        }
    }
    if (contigs) {                                                  /* unitigs + copy plan from the GPU; the handle keeps its own copy of the plan */
        mdbg_unitig_list ul;
        rc = mdbg_graph_unitigs(ctx, &ul);
        if (rc) die(ctx, "mdbg_graph_unitigs", rc);
        printf("Number of unitigs: %llu\n", (unsigned long long)ul.n_unitigs);
        ctg = mdbg_emit_contigs_open(&ul, &nodes, &err);
        if (!ctg) die(NULL, "mdbg_emit_contigs_open", err);
        if (components) {                                           /* of the list just made; the call leaves it as it is */
            mdbg_component_list cl; uint64_t big = 0;
            rc = mdbg_graph_components(ctx, &cl);
            if (rc) die(ctx, "mdbg_graph_components", rc);
            for (uint64_t j = 1; j < cl.n_components; ++j) if (cl.nodes[j] > cl.nodes[big]) big = j;
            printf("components: %llu (largest: %llu nodes, %llu bases)\n", (unsigned long long)cl.n_components, (unsigned long long)(cl.n_components ? cl.nodes[big] : 0),
                   (unsigned long long)(cl.n_components ? cl.bases[big] : 0));
        }
        if (read_paths) {                                           /* of the same list, in bounded ranges of reads; the call leaves the list as it is */
            uint64_t rp_first = 0, with_steps = 0, several = 0, placed = 0, windows = 0;
            for (;;) {
                mdbg_read_path_list rp;
                rc = mdbg_graph_read_paths(ctx, rp_first, (uint64_t)1 << 20, &rp);
                if (rc) die(ctx, "mdbg_graph_read_paths", rc);
                if (!rp.n_reads) break;
                for (uint64_t q = 0; q < rp.n_reads; ++q) {
                    const uint64_t n = rp.step_offsets[q + 1] - rp.step_offsets[q];
                    with_steps += n >= 1; several += n > 1;
                }
                placed += rp.n_placed; windows += rp.n_windows; rp_first += rp.n_reads;
            }
            printf("read paths: %llu reads with a step, %llu / %llu windows placed, %llu reads with more than one step\n", (unsigned long long)with_steps,
                   (unsigned long long)placed, (unsigned long long)windows, (unsigned long long)several);
        }
        if (junctions) {                                            /* of the same list and in the same ranges; the supports of the ranges add up */
            uint64_t jx_first = 0, records = 0, unsupported = 0, crossings = 0, missing = 0;
            uint64_t* support = NULL;
            for (;;) {
                mdbg_junction_list jx;
                rc = mdbg_graph_junctions(ctx, jx_first, (uint64_t)1 << 20, &jx);
                if (rc) die(ctx, "mdbg_graph_junctions", rc);
                if (!jx.n_reads) break;
                if (!support && jx.n_records) {
                    records = jx.n_records;
                    support = (uint64_t*)calloc(records, sizeof *support);
                    if (!support) die(NULL, "calloc", MDBG_E_NOMEM);
                }
                for (uint64_t r = 0; r < jx.n_records; ++r) support[r] += jx.support[r];
                crossings += jx.n_crossings; missing += jx.n_missing_crossings; jx_first += jx.n_reads;
            }
            for (uint64_t r = 0; r < records; ++r) unsupported += support[r] == 0;
            free(support);
            printf("junctions: %llu records, %llu crossed by no read, %llu crossings, %llu of them on no record\n", (unsigned long long)records,
                   (unsigned long long)unsupported, (unsigned long long)crossings, (unsigned long long)missing);
        }
        if (transits) { snprintf(path, sizeof path, "%s.unitigs.transits.tsv", prefix); write_transits(ctx, &ul, path, transits, ""); }
        if (gaf) { snprintf(path, sizeof path, "%s.unitigs.gaf", prefix); write_gaf(ctx, &ul, path, read_lens, ""); }
        if (query) { snprintf(path, sizeof path, "%s.unitigs", prefix); write_query(ctx, &ul, path, query, reference, ""); }
        if (chains) {
            snprintf(path, sizeof path, "%s.unitigs.chains.gaf", prefix); write_chains(ctx, &ul, path, read_lens, chain_skew, chain_gap, "");
            if (query) { snprintf(path, sizeof path, "%s.unitigs", prefix); write_query_chains(ctx, &ul, path, query, reference, chain_skew, chain_gap, ""); }
        }
        if (keep_reads) {
            mdbg_contig_seqs cs;
            rc = mdbg_graph_contigs(ctx, 0, &cs);
            if (rc) die(ctx, "mdbg_graph_contigs", rc);
            rc = mdbg_emit_contigs_set_sequences(ctg, cs.bases, cs.offsets, cs.n_contigs);
            if (rc) die(NULL, "mdbg_emit_contigs_set_sequences", rc);
        }
    }
    if ((write_sequences && !seq_kept) || (ctg && !keep_reads)) {                                   /* second pass over the input: the node sequences, the contigs' bases */
        /* one file per writer thread, "<prefix>.<t>.sequences", as the reference's worker threads write them (main.rs:614-630) */
        enum { MAX_WRITERS = 16 };
        const int nw = !write_sequences || seq_kept ? 0 : threads > MAX_WRITERS ? MAX_WRITERS : threads;
        mdbg_seqfile* sf[MAX_WRITERS]; seqjob_t job[MAX_WRITERS]; pthread_t th[MAX_WRITERS];
        for (int t = 0; t < nw; ++t) {
            snprintf(path, sizeof path, "%s.%d.sequences", prefix, t);
            sf[t] = mdbg_seqfile_open(path, p.k, p.l, &err);
            if (!sf[t]) die(NULL, "mdbg_seqfile_open", err);
        }
        rd = mdbg_reader_open_mt(input, reference, threads, &err);
        if (!rd) die(NULL, "mdbg_reader_open", err);
        first = 0;
        const double ts = now_s();
        for (;;) {
            const uint8_t* bases; const uint64_t* offs; uint64_t n;
            rc = mdbg_reader_next(rd, 256u << 20, &bases, &offs, &n);
            if (rc) die(NULL, "mdbg_reader_next", rc);
            if (!n) break;
            if (ctg && !keep_reads) { rc = mdbg_emit_contigs_add_batch(ctg, bases, offs, n, first); if (rc) die(NULL, "mdbg_emit_contigs_add_batch", rc); }
            if (sctg && !keep_reads) { rc = mdbg_emit_contigs_add_batch(sctg, bases, offs, n, first); if (rc) die(NULL, "mdbg_emit_contigs_add_batch", rc); }
            for (int t = 0; t < nw; ++t) {
                seqjob_t jb; jb.sf = sf[t]; jb.nodes = &nodes; jb.part = (uint32_t)t; jb.n_parts = (uint32_t)nw; jb.bases = bases; jb.offs = offs; jb.n = n; jb.first = first; jb.rc = 0;
                job[t] = jb;
                if (t) pthread_create(&th[t], NULL, seqjob_main, &job[t]);
            }
            if (nw) seqjob_main(&job[0]);
            for (int t = 1; t < nw; ++t) pthread_join(th[t], NULL);
            for (int t = 0; t < nw; ++t) if (job[t].rc) die(NULL, "mdbg_seqfile_write_batch_part", job[t].rc);
            first += n;
        }
        mdbg_reader_close(rd);
        for (int t = 0; t < nw; ++t) { rc = mdbg_seqfile_close(sf[t]); if (rc) die(NULL, "mdbg_seqfile_close", rc); }
        if (timing) fprintf(stderr, "timing: .sequences pass %.3f s (%d file%s)\n", now_s() - ts, nw, nw > 1 ? "s" : "");
    }
    if (ctg) {
        snprintf(path, sizeof path, "%s.unitigs.gfa", prefix);
        rc = mdbg_emit_contigs_write_gfa(ctg, path);
        if (rc) die(NULL, "mdbg_emit_contigs_write_gfa", rc);
        snprintf(path, sizeof path, "%s.unitigs.fa", prefix);
        rc = mdbg_emit_contigs_write_fasta(ctg, path, 0);
        if (rc) die(NULL, "mdbg_emit_contigs_write_fasta", rc);
        mdbg_emit_contigs_close(ctg);
    }
    if (sctg) {
        snprintf(path, sizeof path, "%s.msimpl.gfa", prefix);
        rc = mdbg_emit_contigs_write_gfa(sctg, path);
        if (rc) die(NULL, "mdbg_emit_contigs_write_gfa", rc);
        snprintf(path, sizeof path, "%s.msimpl.fa", prefix);
        rc = mdbg_emit_contigs_write_fasta(sctg, path, 0);
        if (rc) die(NULL, "mdbg_emit_contigs_write_fasta", rc);
        mdbg_emit_contigs_close(sctg);
    }
    free(read_lens);
    mdbg_destroy(ctx);
    return 0;
}
