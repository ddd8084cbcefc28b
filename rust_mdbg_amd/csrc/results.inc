// results.inc — what a context derives from its table and keeps for the caller (the host copy of the node table, the edge list, the unitig list, components, contigs,
// node sequences, read paths, junction support, transits, alignments, chains) and which of it is current.  Knows nothing of the context: included by api.inc in front of context.inc, whose mdbg_ctx holds one Results.
namespace {
// the buffers of one graph stage: created on first use, destroyed with the context
template <class B, B* (*Create)(), void (*Destroy)(B*)> struct StageBuffers {
    std::unique_ptr<B, void (*)(B*)> p{nullptr, Destroy};
    B* get() { if (!p) p.reset(Create()); return p.get(); }
    B* have() const { return p.get(); }      // null while the stage has not run
};
struct EdgeColumns { HostRaw<u32> n1, n2, ov; HostRaw<u8> o1, o2; };      // host copy of an edge list's arrays

// Which derived results (node table <- edge list <- unitig list) an operation ends, each with all that is built on it: whatever changes the table (insertion, clear,
// finalize's setup) ends the node table; an edge call the edge list; an ingest the unitig list (mdbg_graph_contigs).
enum ResultsFrom { FROM_NODES, FROM_EDGES, FROM_UNITIGS };
// the device node table (FinArgs::o_* of mdbg_ctx::finF): NONE no current one; EMPTY the last finalize found nothing resident, its table of no rows is current; ROWS the rows of the last local finalize are intact
enum class NodeTable { NONE, EMPTY, ROWS };

struct Results {
    // ---- per result: the stage's buffers, the last device result, the host copy, the device time of the last call
    struct { HostRaw<u64> keys, shift_full, src_read, src_start, src_end; HostRaw<u32> index, seqlen; HostRaw<u16> abund, shift; HostRaw<u8> rev; } nodes;
    struct { StageBuffers<EdgeBuffers, edge_buffers_create, edge_buffers_destroy> buf; EdgeResult last{}; EdgeColumns h; } edges;      // (buf also sorts for resolve_wrapped)
    struct { StageBuffers<UnitigBuffers, unitig_buffers_create, unitig_buffers_destroy> buf; UnitigResult last{};      // last: of the last unitig / simplify call; contigs, components, read paths and junctions read it
             HostRaw<u64> off, sread, sbegin, dst, length, kc; HostRaw<u32> node, len; HostRaw<u8> ori, rc, circ; EdgeColumns he;
             std::vector<u64> removed_unitigs, removed_nodes, removed_edges; } unitigs;                                  // per-step removal counts of the last mdbg_graph_simplify
    struct { StageBuffers<ComponentBuffers, component_buffers_create, component_buffers_destroy> buf;                    // its result lives until the next component call or simplify call with a component step
             HostRaw<u32> comp, first, unitigs; HostRaw<u64> nodes, bases, kc; HostRaw<u8> circ; } comps;
    struct { StageBuffers<ContigBuffers, contig_buffers_create, contig_buffers_destroy> buf;                             // its result lives until the next contig call (buf also sorts the exceptions of a kept batch)
             HostRaw<u8> bases; HostRaw<u64> off, unitig; double ms = 0; } contigs;
    struct { StageBuffers<NodeSeqBuffers, node_seq_buffers_create, node_seq_buffers_destroy> buf;                        // its result lives until the next node-sequence call
             HostRaw<u8> bases; HostRaw<u64> off; double ms = 0; } nseq;
    struct { StageBuffers<PlacementBuffers, placement_buffers_create, placement_buffers_destroy> buf; } placement;          // holds no result: scratch that any read-path, junction or transit call, or EDGES step of a simplify call, overwrites
    struct { StageBuffers<ReadPathBuffers, read_path_buffers_create, read_path_buffers_destroy> buf;                     // its result lives until the next read-path call
             HostRaw<u64> ord, off, supw, sups; HostRaw<u32> rw, fw, nw, unitig, fe; HostRaw<u8> strand; double ms = 0; } rpaths;
    struct { StageBuffers<JunctionBuffers, junction_buffers_create, junction_buffers_destroy> buf;                       // its result lives until the next junction call or simplify call with an EDGES step
             HostRaw<u64> support, count; HostRaw<u32> u1, e1, u2, e2; HostRaw<u8> s1, s2; double ms = 0; } junctions;
    struct { StageBuffers<TransitBuffers, transit_buffers_create, transit_buffers_destroy> buf;                          // its result lives until the next transit call or simplify call with a REPEATS step
             HostRaw<u64> count, passes; HostRaw<u32> unitig, iu, ie, ou, oe, irec, orec, n_in, n_out; HostRaw<u8> is, os, verdict; double ms = 0; } transits;

    struct { StageBuffers<AlignmentBuffers, alignment_buffers_create, alignment_buffers_destroy> buf;                    // its result lives until the next alignment call; the steps it names are the read-path result's
             HostRaw<u64> aoff, asoff, plen, pbeg, pend; HostRaw<u32> srec, awin, qbeg, qend; double ms = 0; } alns;
    struct { StageBuffers<ChainBuffers, chain_buffers_create, chain_buffers_destroy> buf;                                // its result lives until the next chain call; the alignments it names are the alignment result's
             HostRaw<u64> bent, coff, caoff, plen, pbeg, pend; HostRaw<u32> brec, cwin, cgap, qbeg, qend; double ms = 0; } chains;

    // ---- what is current.  ONLY the functions from here to still_holds write these members; everybody else asks the predicates below.
    struct { NodeTable table = NodeTable::NONE; u64 rows = 0;
             bool edges = false;         // edges.last belongs to the node table as it stands (unitigs.hip reads both)
             bool ulist = false;         // unitigs.last is current: no edge, finalize, ingest, rewind or reset call since
             u64 copies = 0;             // entries of unitigs.last that a REPEATS step of its schedule copied: a table row may then belong to several entries
             bool prefix = false; } cur; // nseq.buf holds the prefix of the rows' lengths of the node table as it stands
    void invalidate(ResultsFrom from) {
        if (from <= FROM_NODES) { cur.table = NodeTable::NONE; cur.prefix = false; }
        if (from <= FROM_EDGES) cur.edges = false;
        cur.ulist = false;
    }
    // A finalize's outcome.  ROWS, and NONE with the rows a partitioned finalize wrote (they are the caller's, no graph stage reads them): what was built on the table
    // before ends.  EMPTY ends nothing: the context is empty, and the empty lists an empty context gives stay current.  The prefix goes with every table.
    void node_table_is(NodeTable t, u64 n) {
        if (t != NodeTable::EMPTY) invalidate(FROM_EDGES);
        cur.table = t; cur.rows = t == NodeTable::ROWS ? n : 0; cur.prefix = false;
    }
    void edge_list_is(const EdgeResult& r, bool current) { edges.last = r; cur.edges = current; }
    void unitig_list_is(const UnitigResult& r, u64 copies = 0) { unitigs.last = r; cur.ulist = true; cur.copies = copies; }
    void prefix_is_summed() { cur.prefix = true; }
    // A temporary batch (mdbg_graph_align_batch) is sketched behind the store, which ends the unitig list as every sketch does, and rolled back: the store is
    // what the list was built on again, and the list is current as it was.  held() before the sketch, still_holds() behind the rollback.
    auto held() const { return cur; }
    void still_holds(const decltype(cur)& before) { cur = before; }

    // The readers ask two DIFFERENT questions about the node table, and the answers differ on a context that holds nothing and was never finalized:
    //   table_or_empty_context  "a table with rows is current, or there is nothing to tabulate": the edge list and the read paths, which answer an empty context with
    //                           empty lists whether or not a finalize has run (so does the unitig list, which looks at `nothing_resident` before any flag);
    //   table_finalized         "a finalize has produced the current table, possibly of no rows": the node sequences, which answer MDBG_E_STATE until then.
    // nothing_resident: no table or no minimizer in the store (nothing_resident(), context.inc).
    bool table_or_empty_context(bool nothing_resident) const { return cur.table == NodeTable::ROWS || nothing_resident; }
    bool table_finalized() const { return cur.table != NodeTable::NONE; }
    bool has_rows_table() const { return cur.table == NodeTable::ROWS; }
    u64 n_rows() const { return has_rows_table() ? cur.rows : 0; }
    bool edge_list_current() const { return has_rows_table() && cur.edges; }
    bool unitig_list_current() const { return cur.ulist; }
    u64 unitig_list_copies() const { return cur.ulist ? cur.copies : 0; }
    bool prefix_summed() const { return cur.prefix; }
};
}  // namespace
