"""End-to-end host pipeline above the two C ABIs: reads file -> GPU hot path -> .gfa + .sequences.

The same stages as rust-mdbg's main() for the default (density) scheme: parse (a reader thread runs ahead of the
GPU like seq_io's reader thread, src/main.rs:830-839), process_read_aux on batches, abundance filter, graph emit
(src/main.rs:1006-1117), and the .sequences file (one LZ4-frame file instead of one per worker thread)."""
import queue
import threading
import time

import numpy as np

from .api import MAGIC_SIMPLIFY_STEPS, MDBG_SIMPLIFY_NESTED, MDBG_SIMPLIFY_REPEATS, Mdbg, edge_columns, junction_text, merge_junctions, merge_transits, read_path_text, transit_self_flags, transit_text, unitig_name
from .align import gaf_append
from .chains import gaf_append_chains
from .emit import Contigs, Emitter, Reader, lmer_filter_from_counts

READ_PATH_CHUNK = 1 << 20      # reads per Mdbg.graph_read_paths / graph_junctions / graph_transits call of run_file


def apply_lmer_counts(m, lmer_counts, l, density, lmer_counts_min, lmer_counts_max):
    """--lmer-counts FILE [--lmer_counts_min A --lmer_counts_max B] (src/main.rs:392-409, 499-503): restrict the sketch of context m"""
    if lmer_counts is None:
        return
    codes, _ = lmer_filter_from_counts(lmer_counts, l, density, lmer_counts_min, lmer_counts_max)
    m.set_lmer_filter(codes)


def run_file(path, prefix, k, l, density, min_abundance=2, reads_already_hpc=False, presimp=0.01, batch_bases=256 << 20,
             strip_newlines=False, device=-1, write_sequences=True, lmer_counts=None, lmer_counts_min=2, lmer_counts_max=100000,
             threads=1, packed=None, contigs=False, simplify=None, keep_reads=False, sequences_from_kept=False, components=False, read_paths=False, junctions=False, transits=0,
             prefilter=False, prefilter_cells=0, gaf=False, query=None, chains=None):
    """-> dict of counters (what the reference prints: reads, nodes before/after filter, edges, presimp removals).
    contigs: also write <prefix>.unitigs.gfa (sequences in the S lines) and <prefix>.unitigs.fa — the unitigs of the graph, compacted on the GPU
    (Mdbg.graph_unitigs) and stitched from the reads in one more pass over the input (shared with the .sequences pass); this is `gfatools asm -u` +
    to_basespace only, no tip or bubble removal.  Adds n_unitigs to the counters.
    simplify (with contigs): a schedule of tip / bubble / superbubble / component / edge-pruning steps, e.g. api.MAGIC_SIMPLIFY_STEPS, api.MAGIC_SUPERBUBBLE_STEPS or [(api.MDBG_SIMPLIFY_EDGES, 1, 0)] + those (the
    sketch store is still resident when the schedule runs, which is all an edge step needs; its count is simplify["total_edges_removed"]) — also write <prefix>.msimpl.gfa / .msimpl.fa, the contigs left after
    Mdbg.graph_simplify(steps) (this project's own order-free rules, not gfatools parity); the .unitigs.* files are unchanged.  Adds n_simplified and simplify (stats).
    A schedule may hold (api.MDBG_SIMPLIFY_NESTED, min_support, 0) steps, repeats steps that may follow a step that copied (a nested repeat needs one step per level), and
    one (api.MDBG_SIMPLIFY_REPEATS, min_support, 0) step, which duplicates the unitigs the resident reads resolve (simplify["entries_copied"]); no read can be
    placed on a list with copies, so with such a step the <prefix>.msimpl.read_paths / .junctions / .transits.tsv files are not written (simplified_read_evidence_written is False).
    components (with contigs): also write <prefix>.unitigs.components.tsv, one line `utgNAME<TAB>component` per unitig: the connected component of the unitig
    graph each unitig lies in (Mdbg.graph_components; numbered by their smallest unitig), and with simplify <prefix>.msimpl.components.tsv for the simplified
    list.  Adds n_components (and n_components_simplified).  The other files are unchanged.
    read_paths (with contigs): also write <prefix>.unitigs.read_paths.tsv, one line `ordinal<TAB>windows<TAB>placed<TAB>path` per read in the order of the store:
    which unitigs the read walks (Mdbg.graph_read_paths; api.read_path_text gives the format), and with simplify <prefix>.msimpl.read_paths.tsv for the
    simplified list.  Adds n_read_steps (and n_read_steps_simplified).  The other files are unchanged.
    junctions (with contigs): also write <prefix>.unitigs.junctions.tsv: per edge record of the unitig list its L line with the number of reads that cross it
    appended, then one X line per place where reads cross and no record exists (Mdbg.graph_junctions; api.junction_text gives the format), and with simplify
    <prefix>.msimpl.junctions.tsv for the simplified list.  Adds n_junction_records, n_junction_records_unsupported, n_crossings and n_missing_crossings (and
    their _simplified twins).  The other files are unchanged.
    transits=N >= 1 (with contigs): also write <prefix>.unitigs.transits.tsv: one T line per (entrance, exit) pair the reads take through a unitig from end to
    end, with its count, then one U line per unitig with two or more entrances and exits saying whether the pairs seen N times or more match them one to one
    (Mdbg.graph_transits; api.transit_text gives the format), and with simplify <prefix>.msimpl.transits.tsv for the simplified list.  Adds n_transits, n_passes,
    n_repeats and n_resolved (and their _simplified twins).  The other files are unchanged.
    gaf (with contigs): also write <prefix>.unitigs.gaf: the reads aligned to the unitig list, one GAF line per alignment (Mdbg.graph_alignments, written by
    libmdbg_emit's mdbg_gaf_append: include/mdbg_align.h gives the columns; qname is the read's ordinal, the reader hands out no names), in the bounded read ranges
    of the read-path writer, and with simplify <prefix>.msimpl.gaf for the simplified list.  Adds n_alignments (and n_alignments_simplified).
    query=PATH (with contigs): sequences that are NOT part of the graph (genes, a reference, contigs), read from PATH with the project's reader in batches and
    aligned to the unitig list without changing it (Mdbg.align_batch): <prefix>.unitigs.query.gaf, and <prefix>.unitigs.query.tsv with one line
    `ordinal<TAB>windows<TAB>placed<TAB>%.2f` per query — its k-min-mers, how many of them lie on the list, and that share in percent (the columns of the
    reference's experiments/amr/parse_hits.py); with simplify the .msimpl. pair.  Adds n_queries, n_query_alignments (and n_query_alignments_simplified).
    chains=(max_skew, max_gap) (with contigs): also write <prefix>.unitigs.chains.gaf: one GAF line per CHAIN, the alignments of a read joined across unplaced windows
    where the graph bridges them (Mdbg.graph_chains, written by libmdbg_emit's mdbg_gaf_append_chains: include/mdbg_chain.h gives the rule, the columns and the tags),
    in the same read ranges, and with simplify <prefix>.msimpl.chains.gaf.  With query= also <prefix>.unitigs.query.chains.gaf and <prefix>.unitigs.query.chains.tsv
    with one line `ordinal<TAB>windows<TAB>placed<TAB>bridged<TAB>%.2f` per query: its k-min-mers, how many lie on the list, how many unplaced ones lie in bridged
    gaps, and the share of (placed + bridged) in percent.  Adds n_chains, n_bridges, n_query_chains, n_query_bridges (and their _simplified twins).  Without it
    every file and every key is what it is without the option.
    keep_reads (with contigs): the context keeps the reads it ingests, packed, on the device (Mdbg(keep_reads=True)) and the contigs' sequences are stitched
    there (Mdbg.graph_contigs) instead of on the host in a second pass: the same files, and without .sequences output the input is read ONCE.
    Adds kept_reads (the store's size) to the counters.
    sequences_from_kept (with write_sequences): the context keeps the reads (whether or not contigs is set) and the .sequences files are written from that
    store right after the edges (Emitter.write_sequences_from_kept: Mdbg.graph_node_seqs in chunks), not in the second pass — which then only runs if the
    contigs still need it (contigs without keep_reads).  Same lines per file, in row order (byte-identical files when the second pass sees the input as one
    batch).  The time goes to seconds_until["sequences_kept"]; "sequences" keeps meaning the second pass and is absent when there is none.  Adds kept_reads.
    prefilter: the reference's --bf, order-free (Mdbg(prefilter=True); include/mdbg_hip.h, MDBG_FLAG_PREFILTER): k-min-mers seen once stay out of the table unless they
    share a filter cell; the same S and L lines up to the node names (DbgEntry.index counts the keys the table holds).  prefilter_cells: 2-bit cells, 0 = 2^32.
    Needs min_abundance >= 2.  Adds n_windows_admitted.
    threads: host threads of the reader (uncompressed input: mdbg_reader_open_mt) and of the 2-bit packer; packed: hand the GPU 2-bit
    packed batches (a quarter of the bytes over PCIe), default: when threads > 1"""
    if packed is None:
        packed = threads > 1
    q = queue.Queue(maxsize=2)
    stop = threading.Event()               # set when the consumer gives up: the reader must not stay blocked in put()

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                pass
        return False

    free = threading.Semaphore(2)          # packed batches are views into the reader's two alternating buffer sets: at most two may be outstanding

    def produce():
        try:
            with Reader(path, strip_newlines, threads=threads, device_buffers=True) as r:
                if packed:
                    # the reader packs while it parses (mdbg_reader_next_packed); batch i+1 is produced while batch i is ingested
                    it = r.batches_packed(batch_bases, copy=False)
                    while True:
                        while not free.acquire(timeout=0.2):
                            if stop.is_set():
                                return
                        pk = next(it, None)
                        if pk is None:
                            break
                        if not put((pk, None, pk["n_bases"])):
                            return
                    put(None)
                    stop.wait()                   # the reader's buffers must outlive the last batch's ingest: wait until the consumer is done
                    return
                if r.parallel:
                    # ASCII batches of the parallel reader are views into its two alternating buffers: no copy, at most two outstanding (as the packed ones);
                    # until round 5 every batch was copied once more on this thread (7 GB of memcpy per 7 Gbases: most of the ASCII path's time)
                    it = r.batches(batch_bases, copy=False)
                    while True:
                        while not free.acquire(timeout=0.2):
                            if stop.is_set():
                                return
                        item = next(it, None)
                        if item is None:
                            break
                        if not put((item[0], item[1].copy(), len(item[0]))):
                            return
                    put(None)
                    stop.wait()
                    return
                for bases, offs in r.batches(batch_bases):
                    if not put((bases, offs, len(bases))):
                        return
            put(None)
        except BaseException as e:          # noqa: BLE001
            put(e)

    th = threading.Thread(target=produce, daemon=True)
    th.start()
    n_reads = n_bases = 0
    read_lens = []                         # gaf: the raw length of every read, from the batch offsets
    tm = {}
    t0 = time.perf_counter()
    try:
        stitched = bool(contigs and keep_reads)      # the contigs' bases come from the device store, not from a second pass
        seq_kept = bool(write_sequences and sequences_from_kept)      # so do the node sequences
        kept = None
        with Mdbg(k, l, density, min_abundance, reads_already_hpc=reads_already_hpc, device=device, keep_reads=stitched or seq_kept, prefilter=prefilter, prefilter_cells=prefilter_cells) as m:
            apply_lmer_counts(m, lmer_counts, l, density, lmer_counts_min, lmer_counts_max)
            tm["open"] = time.perf_counter() - t0
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                payload, offs, nb = item
                if packed:
                    m.ingest_packed(payload, n_reads)
                    free.release()                      # this batch's buffers may be reused
                else:
                    m.ingest(payload, offs, n_reads)    # ctypes releases the GIL: the reader thread parses the next batch meanwhile
                    free.release()
                if gaf or chains is not None:
                    read_lens.append(np.diff(np.asarray(payload["offsets"] if packed else offs).astype(np.uint64)))
                n_reads += (len(payload["offsets"]) if packed else len(offs)) - 1
                n_bases += nb
            tm["ingest"] = time.perf_counter() - t0
            # without the .sequences pass the host needs three columns of the node table (the S lines); the minimizer lists stay on the device, where the edge
            # stage reads them (the full copy-out was 150 MB for 465 k nodes: 40 ms of a 190-ms run)
            nodes = m.finalize(gfa_only=not write_sequences)
            stats = m.stats()
            tm["finalize"] = time.perf_counter() - t0
            # edges on the GPU from the device-resident node table (the reference's single-threaded loop, src/main.rs:1017-1117);
            # the host copy of the list goes straight into the GFA writer
            raw = m.graph_edges(presimp, raw=True)
            edges = dict(n1=[0] * int(raw.n), presimp_removed=int(raw.presimp_removed))
            tm["edges"] = time.perf_counter() - t0
            em = Emitter()
            em.write_gfa(prefix + ".gfa", nodes, raw)
            tm["gfa"] = time.perf_counter() - t0
            if seq_kept:                                 # the node table is current here; the calls below leave it alone, this one leaves them theirs
                t1 = time.perf_counter()
                em.write_sequences_from_kept(prefix, nodes, l, m, threads)
                kept = m.kept_reads()
                tm["sequences_kept"] = time.perf_counter() - t1
            ctg = sctg = sstats = None
            comp = {}

            def write_components(ul, path_, key):        # ul: the context's current unitig list (host arrays): the names need its circular flags
                cc = m.graph_components()
                with open(path_, "w") as f:
                    f.write("".join("%s\t%d\n" % (unitig_name(i, ul.circular[i]), c) for i, c in enumerate(cc["component"].tolist())))
                comp[key] = cc["n_components"]
            def write_read_paths(ul, path_, key):        # the reads in bounded ranges: the call's temporaries grow with the range's minimizers
                comp[key] = 0
                first = 0
                with open(path_, "w") as f:
                    while True:
                        rp = m.graph_read_paths(first, READ_PATH_CHUNK)
                        if not rp["n_reads"]:
                            break
                        f.write(read_path_text(rp, ul.circular))
                        comp[key] += rp["n_steps"]
                        first += rp["n_reads"]
            def write_junctions(ul, path_, suffix):      # the same ranges; supports summed and missing keys merged on the host
                parts, first = [], 0
                while True:
                    jx = m.graph_junctions(first, READ_PATH_CHUNK)
                    if not jx["n_reads"]:
                        break
                    parts.append(jx)
                    first += jx["n_reads"]
                jx = merge_junctions(parts)
                with open(path_, "w") as f:
                    f.write(junction_text(edge_columns(ul.edges), jx["support"], jx, ul.circular))
                comp.update({"n_junction_records" + suffix: jx["n_records"], "n_junction_records_unsupported" + suffix: int((jx["support"] == 0).sum()),
                             "n_crossings" + suffix: jx["n_crossings"], "n_missing_crossings" + suffix: jx["n_missing_crossings"]})
            def write_transits(ul, path_, suffix):       # the same ranges; counts merged by key, the verdicts from the merged counts
                parts, first = [], 0
                while True:
                    tr = m.graph_transits(first, READ_PATH_CHUNK, transits)
                    if not tr["n_reads"]:
                        break
                    parts.append(tr)
                    first += tr["n_reads"]
                tr = merge_transits(parts, transit_self_flags(edge_columns(ul.edges), int(ul.n_unitigs)) if parts else [], transits)
                with open(path_, "w") as f:
                    f.write(transit_text(tr, ul.circular))
                comp.update({f + suffix: tr[f] for f in ("n_transits", "n_passes", "n_repeats", "n_resolved")})
            def write_gaf(ul, path_, key):               # the same ranges; the writer appends range after range
                lens = np.concatenate(read_lens) if read_lens else np.zeros(0, np.uint64)
                open(path_, "w").close()
                comp[key] = 0
                first = 0
                while True:
                    al = m.graph_alignments(first, READ_PATH_CHUNK)
                    if not al["n_reads"]:
                        break
                    gaf_append(path_, al, ul, lens[first:first + al["n_reads"]])
                    comp[key] += al["n_alignments"]
                    first += al["n_reads"]
            def write_query(ul, stem, suffix):           # the query file in the reader's batches: each aligned behind the store and forgotten again
                open(stem + ".query.gaf", "w").close()
                first = n_aln = 0
                with Reader(query, strip_newlines) as qr, open(stem + ".query.tsv", "w") as f:
                    for qb, qo in qr.batches(batch_bases):
                        al = m.align_batch(qb, qo)
                        al["ordinal"] = al["ordinal"] + np.uint64(first)
                        gaf_append(stem + ".query.gaf", al, ul, np.diff(qo.astype(np.uint64)))
                        so = al["step_offsets"].astype(np.int64)
                        placed = np.add.reduceat(np.append(al["step_windows"].astype(np.int64), 0), so[:-1]) * (np.diff(so) > 0) if al["n_reads"] else np.zeros(0, np.int64)
                        f.write("".join("%d\t%d\t%d\t%.2f\n" % (o, w, p, 100.0 * p / w if w else 0.0) for o, w, p in zip(al["ordinal"].tolist(), al["read_windows"].tolist(), placed.tolist())))
                        first += al["n_reads"]
                        n_aln += al["n_alignments"]
                comp["n_queries"] = first
                comp["n_query_alignments" + suffix] = n_aln
            def write_chains(ul, path_, suffix):         # the same ranges, one line per chain
                lens = np.concatenate(read_lens) if read_lens else np.zeros(0, np.uint64)
                open(path_, "w").close()
                comp["n_chains" + suffix] = comp["n_bridges" + suffix] = 0
                first = 0
                while True:
                    ch = m.graph_chains(first, READ_PATH_CHUNK, chains[0], chains[1])
                    n = ch["alignments"]["n_reads"]
                    if not n:
                        break
                    gaf_append_chains(path_, ch, ul, lens[first:first + n])
                    comp["n_chains" + suffix] += ch["n_chains"]
                    comp["n_bridges" + suffix] += ch["n_bridges"]
                    first += n
            def write_query_chains(ul, stem, suffix):    # the query file once more, chained
                open(stem + ".query.chains.gaf", "w").close()
                first = n_chains = n_bridges = 0
                with Reader(query, strip_newlines) as qr, open(stem + ".query.chains.tsv", "w") as f:
                    for qb, qo in qr.batches(batch_bases):
                        ch = m.chain_batch(qb, qo, chains[0], chains[1])
                        al = ch["alignments"]
                        al["ordinal"] = al["ordinal"] + np.uint64(first)
                        gaf_append_chains(stem + ".query.chains.gaf", ch, ul, np.diff(qo.astype(np.uint64)))
                        co = ch["chain_offsets"].astype(np.int64)
                        per_read = lambda col: (np.add.reduceat(np.append(col.astype(np.int64), 0), co[:-1]) * (np.diff(co) > 0)) if al["n_reads"] else np.zeros(0, np.int64)
                        placed, bridged = per_read(ch["chain_windows"]), per_read(ch["chain_gap_windows"])
                        f.write("".join("%d\t%d\t%d\t%d\t%.2f\n" % (o, w, p, g, 100.0 * (p + g) / w if w else 0.0)
                                        for o, w, p, g in zip(al["ordinal"].tolist(), al["read_windows"].tolist(), placed.tolist(), bridged.tolist())))
                        first += al["n_reads"]
                        n_chains += ch["n_chains"]
                        n_bridges += ch["n_bridges"]
                comp["n_query_chains" + suffix] = n_chains
                comp["n_query_bridges" + suffix] = n_bridges
            if contigs and simplify is not None:         # (before the plain list: the handle copies the plan, and graph_unitigs then reuses the buffers)
                sl, sstats = m.graph_simplify(simplify, raw=True)
                sctg = Contigs(sl)
                if components:
                    write_components(sl, prefix + ".msimpl.components.tsv", "n_components_simplified")
                # a REPEATS or NESTED step may leave copies in the list, and no read can be placed on a list with copies: the three read-evidence files of the simplified list are not written
                placeable = not any(int(st[0]) in (MDBG_SIMPLIFY_REPEATS, MDBG_SIMPLIFY_NESTED) for st in simplify)
                comp["simplified_read_evidence_written"] = placeable
                if read_paths and placeable:
                    write_read_paths(sl, prefix + ".msimpl.read_paths.tsv", "n_read_steps_simplified")
                if junctions and placeable:
                    write_junctions(sl, prefix + ".msimpl.junctions.tsv", "_simplified")
                if transits and placeable:
                    write_transits(sl, prefix + ".msimpl.transits.tsv", "_simplified")
                if gaf and placeable:
                    write_gaf(sl, prefix + ".msimpl.gaf", "n_alignments_simplified")
                if query is not None and placeable:
                    write_query(sl, prefix + ".msimpl", "_simplified")
                if chains is not None and placeable:
                    write_chains(sl, prefix + ".msimpl.chains.gaf", "_simplified")
                    if query is not None:
                        write_query_chains(sl, prefix + ".msimpl", "_simplified")
                if stitched:
                    g = m.graph_contigs(0)
                    sctg.set_sequences(g["bases"], g["offsets"])
                tm["simplify"] = time.perf_counter() - t0
            if contigs:                                  # the plan is copied out of the context here; the bases follow in the second pass
                ul = m.graph_unitigs(raw=True)
                ctg = Contigs(ul, nodes["n_nodes"])
                if components:
                    write_components(ul, prefix + ".unitigs.components.tsv", "n_components")
                if read_paths:
                    write_read_paths(ul, prefix + ".unitigs.read_paths.tsv", "n_read_steps")
                if junctions:
                    write_junctions(ul, prefix + ".unitigs.junctions.tsv", "")
                if transits:
                    write_transits(ul, prefix + ".unitigs.transits.tsv", "")
                if gaf:
                    write_gaf(ul, prefix + ".unitigs.gaf", "n_alignments")
                if query is not None:
                    write_query(ul, prefix + ".unitigs", "")
                if chains is not None:
                    write_chains(ul, prefix + ".unitigs.chains.gaf", "")
                    if query is not None:
                        write_query_chains(ul, prefix + ".unitigs", "")
                if stitched:
                    g = m.graph_contigs(0)
                    ctg.set_sequences(g["bases"], g["offsets"])
                    kept = m.kept_reads()
                tm["unitigs"] = time.perf_counter() - t0
        tm["close"] = time.perf_counter() - t0
    finally:
        stop.set()                          # error or not: release the reader (it closes the file) and wait for it
        th.join()
    tm["reader_closed"] = time.perf_counter() - t0
    second_seqs = write_sequences and not seq_kept
    if second_seqs or (ctg is not None and not stitched):               # second pass over the input for the node sequences and the contigs' bases
        def again():
            first = 0
            with Reader(path, strip_newlines, threads=threads) as r:
                for bases, offs in r.batches(batch_bases, copy=False):      # consumed before the next batch is asked for
                    if ctg is not None and not stitched:
                        ctg.add_batch(bases, offs, first)
                    if sctg is not None and not stitched:
                        sctg.add_batch(bases, offs, first)
                    yield bases, offs, first
                    first += len(offs) - 1
        t1 = time.perf_counter()
        if not second_seqs:
            for _ in again():
                pass
        elif threads > 1:                              # one file per writer thread, like the reference's worker threads (main.rs:614-630)
            em.write_sequences_parallel(prefix, nodes, l, again(), min(threads, 16))
        else:
            em.write_sequences(prefix + ".0.sequences", nodes, l, again())
        tm["sequences"] = time.perf_counter() - t1
    extra = dict(comp)
    if kept is not None:
        extra["kept_reads"] = kept
    if ctg is not None:
        with ctg:
            ctg.write_gfa(prefix + ".unitigs.gfa")
            ctg.write_fasta(prefix + ".unitigs.fa")
            extra["n_unitigs"] = len(ctg)
    if sctg is not None:
        with sctg:
            sctg.write_gfa(prefix + ".msimpl.gfa")
            sctg.write_fasta(prefix + ".msimpl.fa")
            extra["n_simplified"] = len(sctg)
            extra["simplify"] = sstats
    if prefilter:
        extra["n_windows_admitted"] = stats["n_windows_admitted"]
    return dict(extra, n_reads=n_reads, n_bases=n_bases, n_minimizers=stats["n_minimizers"], n_windows=stats["n_windows"],
                n_nodes_before=nodes["n_nodes_before"], n_nodes=nodes["n_nodes"], n_edges=len(edges["n1"]),
                presimp_removed=edges["presimp_removed"], seconds_until={k_: round(v, 4) for k_, v in tm.items()})


READ_ORDINAL_BASE = 1 << 32     # contig feedback: the reads' ordinals start here, the contigs of a round take [0, 2 * n_contigs)


def concat_records(seqs):
    """list of bytes -> (uint8 bases, uint64 offsets) as the ingest calls take them"""
    import numpy as np
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offs[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offs


def run_multik(path, prefix, ks, l, density, min_abundance=2, reads_already_hpc=False, presimp=0.01, batch_bases=256 << 20,
               strip_newlines=False, device=-1, contigs_fn=None, min_contig_len=100000, lmer_counts=None, lmer_counts_min=2, lmer_counts_max=100000,
               keep_reads=False, simplify_steps=None, prefilter=False, prefilter_cells=0):
    """One pass over the reads, one graph per k (the k sweep of the reference's utils/multik:69-78): the reads are sketched once,
    the sketches stay resident on the GPU, and every k only clears and refills the counting table (mdbg_reset) and rebuilds nodes
    and edges.  Writes <prefix>-k<k>.gfa; -> {k: counters}.

    contigs_fn(k, gfa_path, nodes) -> list of bytes: the script's contig feedback.  The simplification that turns a round's graph
    into contigs is the caller's (the script shells out to magic_simplify = gfatools + to_basespace, outside this path); what it
    returns is filtered like `seqtk seq -L 100000` (min_contig_len), taken TWICE (`zcat -f x.msimpl.fa x.msimpl.fa`, utils/multik:72)
    and put IN FRONT of the reads for the next k: the reads keep their resident sketches and their ordinals (READ_ORDINAL_BASE + i),
    the contigs get the ordinals 0 .. 2C-1, and the previous round's contigs are forgotten (mdbg_rewind).
    contigs_fn="unitigs": the built-in producer — the round's unitigs (Mdbg.graph_unitigs: `gfatools asm -u` + to_basespace, WITHOUT magic_simplify's tip and
    bubble rounds), stitched from the previous round's contigs and one more pass over the reads per round.
    contigs_fn="simplified": the same with the tip and bubble rounds — the contigs left after Mdbg.graph_simplify(api.MAGIC_SIMPLIFY_STEPS): the schedule of
    magic_simplify's first gfatools line under this project's own rules (include/mdbg_hip.h), not gfatools parity.  simplify_steps: another schedule for that
    producer, e.g. api.MAGIC_SUPERBUBBLE_STEPS (steps that need no resident reads: tips, bubbles, superbubbles, components).
    keep_reads (with the two built-in producers): the reads stay packed on the device (Mdbg(keep_reads=True)); a round's contigs are stitched there
    (mdbg_graph_contigs_device(min_contig_len)) and ingested for the next round straight from that device buffer, twice, with first ordinals 0 and C — the
    ordinals the concatenated contigs + contigs batch gives.  No Reader is opened after the first pass; same counters, same files.
    prefilter, prefilter_cells: every round with the counting pre-filter (the script runs `--minabund 2 --bf`), see run_file: the filter is counted anew per k and
    per round's contigs."""
    import ctypes
    ks = list(ks)
    schedule = MAGIC_SIMPLIFY_STEPS if simplify_steps is None else list(simplify_steps)
    on_device = bool(keep_reads and contigs_fn in ("unitigs", "simplified"))
    out = {}
    n_reads = n_bases = 0
    base = READ_ORDINAL_BASE if contigs_fn is not None else 0
    with Mdbg(ks[0], l, density, min_abundance, reads_already_hpc=reads_already_hpc, device=device, keep_reads=on_device, prefilter=prefilter, prefilter_cells=prefilter_cells) as m, Reader(path, strip_newlines) as r:
        apply_lmer_counts(m, lmer_counts, l, density, lmer_counts_min, lmer_counts_max)
        for bases, offs in r.batches(batch_bases):
            m.ingest(bases, offs, base + n_reads)
            n_reads += len(offs) - 1
            n_bases += len(bases)
        mark = m.mark()
        em = Emitter()
        contigs = []
        dev_contigs = None                               # on_device: (d_bases, d_offsets, C, n_bases) of the last round's contigs, owned by the context
        for i, k in enumerate(ks):
            if i:
                if contigs_fn is not None:
                    m.rewind(mark)                       # last round's contigs go, the reads' sketches stay
                m.reset(k)                               # sketches stay; windows of the new k are inserted again
                if dev_contigs is not None and dev_contigs[2]:
                    db, do, nc, nb = dev_contigs         # (the buffers live until the next graph_contigs call; a keeping context copies what it ingests)
                    m.ingest_device(db, do, nc, nb, 0)
                    m.ingest_device(db, do, nc, nb, nc)
                if contigs:
                    twice = contigs + contigs
                    cb, co = concat_records(twice)
                    m.ingest(cb, co, 0)
            nodes = m.finalize()
            raw = m.graph_edges(presimp, raw=True)
            gfa = "%s-k%d.gfa" % (prefix, k)
            em.write_gfa(gfa, nodes, raw)
            st = m.stats()
            out[k] = dict(n_reads=n_reads, n_bases=n_bases, n_contigs=dev_contigs[2] if dev_contigs is not None else len(contigs), n_minimizers=st["n_minimizers"], n_windows=st["n_windows"],
                          n_nodes_before=nodes["n_nodes_before"], n_nodes=nodes["n_nodes"], n_edges=int(raw.n),
                          presimp_removed=int(raw.presimp_removed))
            if on_device:
                if contigs_fn == "unitigs":
                    m.graph_unitigs_device()
                else:
                    m.graph_simplify_device(schedule)
                cs = m.graph_contigs(min_contig_len, device=True)
                dev_contigs = (ctypes.cast(cs.bases, ctypes.c_void_p).value or 0, ctypes.cast(cs.offsets, ctypes.c_void_p).value or 0, int(cs.n_contigs), int(cs.n_bases))
            elif contigs_fn in ("unitigs", "simplified"):
                def fed():                               # what this round ingested, with its ordinals: the contigs in front, then the reads
                    if contigs:
                        yield concat_records(contigs + contigs) + (0,)
                    first = base
                    with Reader(path, strip_newlines) as r2:
                        for bases, offs in r2.batches(batch_bases, copy=False):
                            yield bases, offs, first
                            first += len(offs) - 1
                plan, n_nodes = (m.graph_unitigs(raw=True), nodes["n_nodes"]) if contigs_fn == "unitigs" else (m.graph_simplify(schedule, raw=True)[0], None)
                with em.contigs(plan, fed(), n_nodes=n_nodes) as ctg:
                    contigs = [c for c in ctg.sequences() if len(c) >= min_contig_len]
            elif contigs_fn is not None:
                contigs = [bytes(c) for c in contigs_fn(k, gfa, nodes) if len(c) >= min_contig_len]
    return out
