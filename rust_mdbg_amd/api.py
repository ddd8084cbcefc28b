"""ctypes binding of include/mdbg_hip.h — the host-side mirror of rust-mdbg's per-read path.

Names follow the reference: `Params` (src/main.rs:92-114), `Mdbg.ingest` = process_read_aux over a batch
(src/main.rs:730-785), `Mdbg.sketch` = Read::extract (src/read.rs:85-90), `Mdbg.finalize` = the abundance filter
plus the read-only node view the graph emitter walks (src/main.rs:922-929,1014-1016).
"""
import ctypes as C
import os

import numpy as np

from . import align as _align
from . import chains as _chains

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MDBG_OK, MDBG_E_PARAM, MDBG_E_ALPHABET, MDBG_E_CAPACITY, MDBG_E_DEVICE, MDBG_E_NOMEM, MDBG_E_STATE, MDBG_E_IO = 0, -1, -2, -3, -4, -5, -6, -7
FLAG_FORCE_GENERIC = 1   # mdbg_params.flags bit 0: every tile takes the generic exact kernel (testing)
FLAG_KEEP_READS = 2      # mdbg_params.flags bit 1: the context keeps the reads it ingests, packed, on the device (Mdbg.graph_contigs)
FLAG_PREFILTER = 4       # mdbg_params.flags bit 2: the counting pre-filter in front of the node table (--bf made order-free; include/mdbg_hip.h, MDBG_FLAG_PREFILTER)


class MdbgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mdbg error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("l", C.c_uint32), ("density", C.c_double), ("min_abundance", C.c_uint32),
                ("reads_already_hpc", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("table_capacity_hint", C.c_uint64), ("scheme", C.c_uint32), ("syncmer_s", C.c_uint32), ("prefilter_cells", C.c_uint64),
                ("reserved", C.c_uint64 * 2)]


class Nodes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("keys", C.POINTER(C.c_uint64)), ("index", C.POINTER(C.c_uint32)),
                ("abundance", C.POINTER(C.c_uint16)), ("seqlen", C.POINTER(C.c_uint32)), ("shift", C.POINTER(C.c_uint16)),
                ("shift_full", C.POINTER(C.c_uint64)), ("src_read", C.POINTER(C.c_uint64)), ("src_start", C.POINTER(C.c_uint64)),
                ("src_end", C.POINTER(C.c_uint64)), ("reversed", C.POINTER(C.c_uint8)), ("n_distinct", C.c_uint64),
                ("n_wrapped", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_minimizers", C.c_uint64), ("n_windows", C.c_uint64),
                ("n_distinct", C.c_uint64), ("table_capacity", C.c_uint64), ("n_slow_tiles", C.c_uint64), ("n_tiles", C.c_uint64),
                ("ms_sketch", C.c_double), ("ms_insert", C.c_double), ("ms_finalize", C.c_double), ("ms_sketch_tile", C.c_double),
                ("n_sketch_tile_launches", C.c_uint64), ("n_sketch_tile_bases", C.c_uint64), ("tile_bases", C.c_uint64),
                ("n_link_matches", C.c_uint64), ("n_windows_admitted", C.c_uint64), ("prefilter_cells", C.c_uint64), ("reserved", C.c_uint64 * 1)]


class RoutedLists(C.Structure):
    _fields_ = [("n_all", C.c_uint64), ("n_solid", C.c_uint64), ("d_first", C.c_void_p), ("d_solid", C.c_void_p), ("d_ath", C.c_void_p),
                ("d_count", C.c_void_p), ("d_slot", C.c_void_p), ("d_idx_all", C.c_void_p), ("counts_all", C.c_uint64 * 64),
                ("counts_solid", C.c_uint64 * 64)]


class SketchStore(C.Structure):
    _fields_ = [("n_minimizers", C.c_uint64), ("n_reads", C.c_uint64), ("d_hashes", C.c_void_p), ("d_positions", C.c_void_p),
                ("d_read_offsets", C.c_void_p)]


class BatchInfo(C.Structure):
    _fields_ = [("store_offset", C.c_uint64), ("n_minimizers", C.c_uint64), ("first_slot", C.c_uint64), ("n_reads", C.c_uint64),
                ("first_read_ordinal", C.c_uint64), ("d_hashes", C.c_void_p), ("d_positions", C.c_void_p), ("d_read_offsets", C.c_void_p)]


class EdgeList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n1", C.POINTER(C.c_uint32)), ("o1", C.POINTER(C.c_uint8)), ("n2", C.POINTER(C.c_uint32)),
                ("o2", C.POINTER(C.c_uint8)), ("overlap", C.POINTER(C.c_uint32)), ("presimp_removed", C.c_uint64)]


class UnitigList(C.Structure):           # mdbg_unitig_list
    _fields_ = [("n_unitigs", C.c_uint64), ("n_entries", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("node", C.POINTER(C.c_uint32)),
                ("ori", C.POINTER(C.c_uint8)), ("src_read", C.POINTER(C.c_uint64)), ("src_begin", C.POINTER(C.c_uint64)), ("len", C.POINTER(C.c_uint32)),
                ("revcomp", C.POINTER(C.c_uint8)), ("dst_offset", C.POINTER(C.c_uint64)), ("length", C.POINTER(C.c_uint64)),
                ("kc_sum", C.POINTER(C.c_uint64)), ("circular", C.POINTER(C.c_uint8)), ("edges", EdgeList), ("n_rounds", C.c_uint32),
                ("reserved", C.c_uint32)]


UNITIG_FIELDS = (("offsets", np.uint64), ("node", np.uint32), ("ori", np.uint8), ("src_read", np.uint64), ("src_begin", np.uint64), ("len", np.uint32),
                 ("revcomp", np.uint8), ("dst_offset", np.uint64), ("length", np.uint64), ("kc_sum", np.uint64), ("circular", np.uint8))
EDGE_FIELDS = (("n1", np.uint32), ("o1", np.uint8), ("n2", np.uint32), ("o2", np.uint8), ("overlap", np.uint32))


def unitig_counts(u):
    """elements of every array of a UnitigList, by field name"""
    nu, ne = int(u.n_unitigs), int(u.n_entries)
    return dict(offsets=nu + 1 if nu else 0, node=ne, ori=ne, src_read=ne, src_begin=ne, len=ne, revcomp=ne, dst_offset=ne, length=nu, kc_sum=nu, circular=nu)


class ComponentList(C.Structure):      # mdbg_component_list
    _fields_ = [("n_unitigs", C.c_uint64), ("n_components", C.c_uint64), ("component", C.POINTER(C.c_uint32)), ("first_unitig", C.POINTER(C.c_uint32)),
                ("unitigs", C.POINTER(C.c_uint32)), ("nodes", C.POINTER(C.c_uint64)), ("bases", C.POINTER(C.c_uint64)), ("kc_sum", C.POINTER(C.c_uint64)),
                ("circular", C.POINTER(C.c_uint8))]


# (field, dtype, per unitig rather than per component)
COMPONENT_FIELDS = (("component", np.uint32, True), ("first_unitig", np.uint32, False), ("unitigs", np.uint32, False), ("nodes", np.uint64, False),
                    ("bases", np.uint64, False), ("kc_sum", np.uint64, False), ("circular", np.uint8, False))


class ReadPathList(C.Structure):       # mdbg_read_path_list
    _fields_ = [("first_read", C.c_uint64), ("n_reads", C.c_uint64), ("n_windows", C.c_uint64), ("n_placed", C.c_uint64), ("n_steps", C.c_uint64),
                ("n_unitigs", C.c_uint64), ("ordinal", C.POINTER(C.c_uint64)), ("read_windows", C.POINTER(C.c_uint32)), ("step_offsets", C.POINTER(C.c_uint64)), ("first_window", C.POINTER(C.c_uint32)),
                ("step_windows", C.POINTER(C.c_uint32)), ("unitig", C.POINTER(C.c_uint32)), ("first_entry", C.POINTER(C.c_uint32)), ("strand", C.POINTER(C.c_uint8)),
                ("support_windows", C.POINTER(C.c_uint64)), ("support_steps", C.POINTER(C.c_uint64))]


# (field, dtype, what it has one element of: "read", "step" or "unitig")
READ_PATH_FIELDS = (("ordinal", np.uint64, "read"), ("read_windows", np.uint32, "read"), ("first_window", np.uint32, "step"), ("step_windows", np.uint32, "step"), ("unitig", np.uint32, "step"),
                    ("first_entry", np.uint32, "step"), ("strand", np.uint8, "step"), ("support_windows", np.uint64, "unitig"), ("support_steps", np.uint64, "unitig"))


# the columns of Mdbg.graph_alignments / align_batch (include/mdbg_align.h), in the style of READ_PATH_FIELDS: (field, dtype, "read" / "step" / "alignment")
ALIGNMENT_FIELDS, ALIGNMENT_OFFSETS, ALIGNMENT_COUNTS = _align.ALIGNMENT_FIELDS, _align.ALIGNMENT_OFFSETS, _align.ALIGNMENT_COUNTS


def read_path_text(rp, circular):
    """the lines of a .read_paths.tsv for a graph_read_paths() result: one per read in slot order, `ordinal<TAB>windows<TAB>placed<TAB>path`; path is `*` for a read
    without steps, else its steps joined by `,`, each `first_window:n_windows:>NAME:first_entry` (`<` for strand 1) with NAME the unitig's utg%07d[lc] name.
    circular: the list's `circular` array.  (windows of a read = the windows its minimizers give, placed = the sum over its steps.)"""
    off = rp["step_offsets"].tolist()
    fw, nw, un, fe, st = (rp[f].tolist() for f in ("first_window", "step_windows", "unitig", "first_entry", "strand"))
    lines = []
    for q, o in enumerate(rp["ordinal"].tolist()):
        steps = range(off[q], off[q + 1])
        path = ",".join("%d:%d:%s%s:%d" % (fw[p], nw[p], "<" if st[p] else ">", unitig_name(un[p], circular[un[p]]), fe[p]) for p in steps) or "*"
        lines.append("%d\t%d\t%d\t%s\n" % (o, rp["read_windows"][q], sum(nw[p] for p in steps), path))
    return "".join(lines)


class JunctionList(C.Structure):       # mdbg_junction_list
    _fields_ = [("first_read", C.c_uint64), ("n_reads", C.c_uint64), ("n_adjacent", C.c_uint64), ("n_links", C.c_uint64), ("n_crossings", C.c_uint64),
                ("n_explained", C.c_uint64), ("n_missing_crossings", C.c_uint64), ("n_records", C.c_uint64), ("n_missing", C.c_uint64),
                ("support", C.POINTER(C.c_uint64)), ("missing_unitig1", C.POINTER(C.c_uint32)), ("missing_entry1", C.POINTER(C.c_uint32)),
                ("missing_strand1", C.POINTER(C.c_uint8)), ("missing_unitig2", C.POINTER(C.c_uint32)), ("missing_entry2", C.POINTER(C.c_uint32)),
                ("missing_strand2", C.POINTER(C.c_uint8)), ("missing_count", C.POINTER(C.c_uint64))]


# (field, dtype, what it has one element of: "record" or "missing")
JUNCTION_FIELDS = (("support", np.uint64, "record"), ("missing_unitig1", np.uint32, "missing"), ("missing_entry1", np.uint32, "missing"), ("missing_strand1", np.uint8, "missing"),
                   ("missing_unitig2", np.uint32, "missing"), ("missing_entry2", np.uint32, "missing"), ("missing_strand2", np.uint8, "missing"), ("missing_count", np.uint64, "missing"))
JUNCTION_COUNTS = ("n_reads", "n_adjacent", "n_links", "n_crossings", "n_explained", "n_missing_crossings")      # what adds up over the ranges of a partition of the reads
MISSING_COLUMNS = tuple(f for f, _, per in JUNCTION_FIELDS if per == "missing")


def junction_text(edges, support, missing, circular):
    """the lines of a .junctions.tsv: first one per edge record of the unitig list in list order, the record's L line of the .gfa with the number of reads that cross it
    appended, `L<TAB>utgA<TAB>o1<TAB>utgB<TAB>o2<TAB>overlapM<TAB>support`; then one per missing key in key order, a place where reads cross and no record exists,
    `X<TAB>utgA<TAB>+|-<TAB>entry1<TAB>utgB<TAB>+|-<TAB>entry2<TAB>count` (`+` = strand 0).  edges: the list's `edges` dict; support: per record; missing: a dict with
    the seven missing_* columns (a graph_junctions() result, or the merge of several); circular: the list's `circular` array."""
    name = lambda u: unitig_name(u, circular[u])
    sign = lambda s: "-" if s else "+"
    n1, o1, n2, o2, ov = (np.asarray(edges[f]).tolist() for f, _ in EDGE_FIELDS)
    lines = ["L\t%s\t%s\t%s\t%s\t%dM\t%d\n" % (name(a), chr(oa), name(b), chr(ob), v, s) for a, oa, b, ob, v, s in zip(n1, o1, n2, o2, ov, np.asarray(support).tolist())]
    for u1, j1, s1, u2, j2, s2, n in zip(*(np.asarray(missing[f]).tolist() for f in MISSING_COLUMNS)):
        lines.append("X\t%s\t%s\t%d\t%s\t%s\t%d\t%d\n" % (name(u1), sign(s1), j1, name(u2), sign(s2), j2, n))
    return "".join(lines)


def merge_junctions(parts):
    """the graph_junctions() results of the ranges of a partition of the reads -> the whole call's: the counts and the supports add up, the missing lists merge by
    key (counts added, ascending key order)"""
    parts = list(parts)
    out = {f: sum(p[f] for p in parts) for f in JUNCTION_COUNTS}
    with_records = [p for p in parts if p["n_records"]]            # (a range behind the store, an empty list: no arrays)
    out["n_records"] = with_records[0]["n_records"] if with_records else 0
    out["support"] = sum((p["support"] for p in with_records), np.zeros(out["n_records"], np.uint64))
    by_key = {}
    for p in parts:
        for row in zip(*(p[f].tolist() for f in MISSING_COLUMNS)):
            by_key[row[:6]] = by_key.get(row[:6], 0) + row[6]
    rows = [key + (by_key[key],) for key in sorted(by_key)]       # (tuples of the six columns compare as keys do)
    for i, (f, t, _) in enumerate(JUNCTION_FIELDS[1:]):
        out[f] = np.array([r[i] for r in rows], dtype=t)
    out.update(first_read=parts[0]["first_read"] if parts else 0, n_missing=len(rows))
    return out


class TransitList(C.Structure):        # mdbg_transit_list
    _fields_ = [("first_read", C.c_uint64), ("n_reads", C.c_uint64), ("n_crossings", C.c_uint64), ("n_explained", C.c_uint64), ("n_passes", C.c_uint64),
                ("n_transits", C.c_uint64), ("n_unitigs", C.c_uint64), ("n_repeats", C.c_uint64), ("n_resolved", C.c_uint64),
                ("unitig", C.POINTER(C.c_uint32)), ("in_unitig", C.POINTER(C.c_uint32)), ("in_entry", C.POINTER(C.c_uint32)), ("in_strand", C.POINTER(C.c_uint8)),
                ("out_unitig", C.POINTER(C.c_uint32)), ("out_entry", C.POINTER(C.c_uint32)), ("out_strand", C.POINTER(C.c_uint8)),
                ("in_record", C.POINTER(C.c_uint32)), ("out_record", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint64)),
                ("n_in", C.POINTER(C.c_uint32)), ("n_out", C.POINTER(C.c_uint32)), ("passes", C.POINTER(C.c_uint64)), ("verdict", C.POINTER(C.c_uint8))]


# (field, dtype, what it has one element of: "transit" or "unitig")
TRANSIT_FIELDS = (("unitig", np.uint32, "transit"), ("in_unitig", np.uint32, "transit"), ("in_entry", np.uint32, "transit"), ("in_strand", np.uint8, "transit"),
                  ("out_unitig", np.uint32, "transit"), ("out_entry", np.uint32, "transit"), ("out_strand", np.uint8, "transit"), ("in_record", np.uint32, "transit"),
                  ("out_record", np.uint32, "transit"), ("count", np.uint64, "transit"),
                  ("n_in", np.uint32, "unitig"), ("n_out", np.uint32, "unitig"), ("passes", np.uint64, "unitig"), ("verdict", np.uint8, "unitig"))
TRANSIT_COUNTS = ("n_reads", "n_crossings", "n_explained", "n_passes")      # what adds up over the ranges of a partition of the reads
TRANSIT_COLUMNS = tuple(f for f, _, per in TRANSIT_FIELDS if per == "transit")
TRANSIT_PLAIN, TRANSIT_RESOLVED, TRANSIT_UNRESOLVED, TRANSIT_SELF = 0, 1, 2, 3      # MDBG_TRANSIT_*
TRANSIT_VERDICT_NAMES = ("plain", "resolved", "unresolved", "self")


def transit_verdicts(n_in, n_out, self_flags, merged, min_support):
    """the verdict rule of mdbg_graph_transits on the host, for counts merged over ranges: n_in, n_out per unitig (any range's: they depend on the records alone),
    self_flags per unitig (some record has n1 == n2 == u), merged: a dict with the row columns (a graph_transits() result or merge_transits' of several)
    -> verdict u8[n_unitigs]"""
    assert min_support >= 1
    strong = {}
    for u, pu, pj, ps, qu, qj, qs, n in zip(*(np.asarray(merged[f]).tolist() for f in TRANSIT_COLUMNS[:7] + ("count",))):
        if n >= min_support:
            strong.setdefault(u, []).append(((pu, pj, ps), (qu, qj, qs)))
    out = np.zeros(len(n_in), np.uint8)
    for u, (ni, no, own) in enumerate(zip(np.asarray(n_in).tolist(), np.asarray(n_out).tolist(), np.asarray(self_flags).tolist())):
        if ni < 2 or no < 2:
            continue
        s = strong.get(u, [])
        matched = ni == no == len(s) and len({p for p, _ in s}) == len(s) and len({q for _, q in s}) == len(s)
        out[u] = TRANSIT_SELF if own else TRANSIT_RESOLVED if matched else TRANSIT_UNRESOLVED
    return out


def transit_self_flags(edges, n_unitigs):
    """per unitig: 1 iff some record of the list's `edges` has n1 == n2 == u"""
    n1, n2 = np.asarray(edges["n1"]), np.asarray(edges["n2"])
    out = np.zeros(n_unitigs, np.uint8)
    out[n1[n1 == n2]] = 1
    return out


def merge_transits(parts, self_flags=None, min_support=1):
    """the graph_transits() results of the ranges of a partition of the reads -> the whole call's: the rows merge by key (counts added, key order kept), passes and
    the counts that are sums add up.  Verdicts belong to their range: with self_flags (transit_self_flags of the list's edges) they are computed again on the merged
    counts by transit_verdicts, and n_repeats / n_resolved with them; without, the result carries no verdict."""
    parts = list(parts)
    out = {f: sum(p[f] for p in parts) for f in TRANSIT_COUNTS}
    with_unitigs = [p for p in parts if p["n_unitigs"]]           # (a range behind the store, an empty list: no arrays)
    U = with_unitigs[0]["n_unitigs"] if with_unitigs else 0
    by_key = {}
    for p in parts:
        for row in zip(*(p[f].tolist() for f in TRANSIT_COLUMNS)):
            at = by_key.setdefault(row[:7], [row[7], row[8], 0])   # (the two records follow from the key)
            at[2] += row[9]
    rows = [key + tuple(by_key[key]) for key in sorted(by_key)]   # (tuples of the seven columns compare as keys do)
    for i, (f, t, _) in enumerate(TRANSIT_FIELDS[:10]):
        out[f] = np.array([r[i] for r in rows], dtype=t)
    out["n_in"] = with_unitigs[0]["n_in"].copy() if with_unitigs else np.zeros(0, np.uint32)
    out["n_out"] = with_unitigs[0]["n_out"].copy() if with_unitigs else np.zeros(0, np.uint32)
    out["passes"] = sum((p["passes"] for p in with_unitigs), np.zeros(U, np.uint64))
    out.update(first_read=parts[0]["first_read"] if parts else 0, n_transits=len(rows), n_unitigs=U)
    if self_flags is not None:
        out["verdict"] = transit_verdicts(out["n_in"], out["n_out"], self_flags, out, min_support)
        repeat = (out["n_in"] >= 2) & (out["n_out"] >= 2)
        out.update(n_repeats=int(repeat.sum()), n_resolved=int((out["verdict"] == TRANSIT_RESOLVED).sum()))
    return out


def transit_text(t, circular):
    """the lines of a .transits.tsv: first one per transit key in key order, `T<TAB>utgA<TAB>+|-<TAB>utgU<TAB>+<TAB>utgB<TAB>+|-<TAB>count` — reads enter unitig U from
    A and leave it for B count times; the signs of A and B are the strands of p and q (`+` = strand 0), so the line reads as the two L lines `A oA U +` and
    `U + B oB` —, then one per unitig with n_in >= 2 and n_out >= 2 in unitig order, `U<TAB>utgU<TAB>n_in<TAB>n_out<TAB>passes<TAB>plain|resolved|unresolved|self`.
    t: a graph_transits() result or merge_transits' with verdicts; circular: the list's `circular` array."""
    name = lambda u: unitig_name(u, circular[u])
    sign = lambda s: "-" if s else "+"
    cols = [np.asarray(t[f]).tolist() for f in ("unitig", "in_unitig", "in_strand", "out_unitig", "out_strand", "count")]
    lines = ["T\t%s\t%s\t%s\t+\t%s\t%s\t%d\n" % (name(a), sign(sa), name(u), name(b), sign(sb), n) for u, a, sa, b, sb, n in zip(*cols)]
    for u, (ni, no, n, v) in enumerate(zip(*(np.asarray(t[f]).tolist() for f in ("n_in", "n_out", "passes", "verdict")))):
        if ni >= 2 and no >= 2:
            lines.append("U\t%s\t%d\t%d\t%d\t%s\n" % (name(u), ni, no, n, TRANSIT_VERDICT_NAMES[v]))
    return "".join(lines)


class ContigSeqs(C.Structure):         # mdbg_contig_seqs
    _fields_ = [("n_contigs", C.c_uint64), ("n_bases", C.c_uint64), ("bases", C.POINTER(C.c_uint8)), ("offsets", C.POINTER(C.c_uint64)),
                ("unitig", C.POINTER(C.c_uint64))]


class NodeSeqs(C.Structure):           # mdbg_node_seqs
    _fields_ = [("first_row", C.c_uint64), ("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("bases", C.POINTER(C.c_uint8)), ("offsets", C.POINTER(C.c_uint64))]


class SimplifyStep(C.Structure):       # mdbg_simplify_step
    _fields_ = [("kind", C.c_uint32), ("max_nodes", C.c_uint32), ("max_bases", C.c_uint64)]


class SimplifyStats(C.Structure):      # mdbg_simplify_stats
    _fields_ = [("n_steps", C.c_uint32), ("n_compactions", C.c_uint32), ("unitigs_removed", C.POINTER(C.c_uint64)), ("nodes_removed", C.POINTER(C.c_uint64)),
                ("total_unitigs_removed", C.c_uint64), ("total_nodes_removed", C.c_uint64), ("n_rounds_total", C.c_uint32), ("n_syncs", C.c_uint32)]


MDBG_SIMPLIFY_TIPS, MDBG_SIMPLIFY_BUBBLES = 1, 2
MDBG_SIMPLIFY_COMPONENTS = 4      # (kind, max_nodes, max_bases): every unitig of a non-circular connected component of at most max_nodes nodes and max_bases bases goes
MDBG_SIMPLIFY_EDGES = 8           # (kind, min_support, 0): every edge record crossed by fewer than min_support resident reads goes where reads leave its source and enter its target another way
MDBG_SIMPLIFY_REPEATS = 16        # (kind, min_support, 0): every unitig the resident reads resolve at min_support (graph_transits) is duplicated, one copy per strong key; at most one per schedule, no EDGES step behind it
MDBG_SIMPLIFY_NESTED = 128        # (kind, min_support, 0): a repeats step that may stand behind a REPEATS step or another NESTED step: the reads are placed on the list with its copies, so a repeat that only exists once its middle is resolved is resolved too; no EDGES or REPEATS step behind it
MDBG_SIMPLIFY_SUPERBUBBLES = 64   # (kind, max_nodes, max_bases): every bubble whose inside may branch (at most max_nodes entries and max_bases bases inside, 0 = no limit) keeps the path whose weakest unitig is strongest
MDBG_SUPERBUBBLE_MAX_UNITIGS = 64 # the unitigs inside one such bubble
_T, _B = (MDBG_SIMPLIFY_TIPS, 10, 50000), (MDBG_SIMPLIFY_BUBBLES, 0, 100000)
# the schedule of the first `gfatools asm` line of utils/magic_simplify, as (kind, max_nodes, max_bases): -t N,L = tips of at most N nodes and L bases,
# -b L = bubbles whose branches have at most L bases.  Same schedule, this project's own order-free rules (include/mdbg_hip.h): not gfatools parity.
MAGIC_SIMPLIFY_STEPS = [_T, _T, _B, _B, _T, _B, _B, _B, _T, _B, _T, (MDBG_SIMPLIFY_BUBBLES, 0, 1000000), (MDBG_SIMPLIFY_TIPS, 10, 150000),
                        (MDBG_SIMPLIFY_BUBBLES, 0, 1000000)]
# the same schedule with every bubble step as a superbubble step with the same limits (they then bound the bubble's inside, not one branch)
MAGIC_SUPERBUBBLE_STEPS = [(MDBG_SIMPLIFY_SUPERBUBBLES, mn, mb) if kind == MDBG_SIMPLIFY_BUBBLES else (kind, mn, mb) for kind, mn, mb in MAGIC_SIMPLIFY_STEPS]


def simplify_steps(steps):
    """[(kind, max_nodes, max_bases)] -> (ctypes array of mdbg_simplify_step or None, n)"""
    steps = [tuple(int(x) for x in s) for s in steps]
    if not steps:
        return None, 0
    return (SimplifyStep * len(steps))(*[SimplifyStep(k, mn, mb) for k, mn, mb in steps]), len(steps)


def unitig_name(i, circular):
    """name of unitig i (0-based) as the writers print it: the shape of gfatools' names quoted in src/to_basespace.rs:89,103,294"""
    return "utg%07d%s" % (i + 1, "c" if circular else "l")


class PackedBatch(C.Structure):          # mdbg_packed_batch
    _fields_ = [("words", C.c_void_p), ("offsets", C.c_void_p), ("n_reads", C.c_uint64), ("exc_pos", C.c_void_p),
                ("exc_val", C.c_void_p), ("n_exc", C.c_uint64)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("genome_len", C.c_uint64), ("n_reads", C.c_uint64), ("mean_len", C.c_uint32),
                ("sd_len", C.c_uint32), ("min_len", C.c_uint32), ("max_len", C.c_uint32), ("err_ppm", C.c_uint32),
                ("reserved", C.c_uint32)]


EXPORTS = ["mdbg_abi_version", "mdbg_build_flags", "mdbg_create", "mdbg_destroy", "mdbg_finalize_device", "mdbg_finalize_gfa", "mdbg_nodes_digest", "mdbg_set_timing", "mdbg_ingest_batch", "mdbg_ingest_batch_device", "mdbg_sketch_only",
           "mdbg_finalize", "mdbg_reset", "mdbg_get_stats", "mdbg_strerror", "mdbg_last_error", "mdbg_sketch_device",
           "mdbg_insert_resident", "mdbg_route_pack", "mdbg_insert_records", "mdbg_sync", "mdbg_synth_reads_device", "mdbg_copy_to_host", "mdbg_copy_to_device",
           "mdbg_routed_export", "mdbg_resolve_first", "mdbg_resolve_meta", "mdbg_routed_keys", "mdbg_arena_reserve",
           "mdbg_set_partition", "mdbg_sketch_view", "mdbg_ingest_sketch", "mdbg_finalize_begin", "mdbg_finalize_end",
           "mdbg_store_reserve", "mdbg_sketch_reserve", "mdbg_sketch_commit", "mdbg_last_batch", "mdbg_owner_counts", "mdbg_graph_edges", "mdbg_graph_edges_device", "mdbg_graph_unitigs", "mdbg_graph_unitigs_device",
           "mdbg_graph_simplify", "mdbg_graph_simplify_device", "mdbg_simplify_edges_removed", "mdbg_graph_components", "mdbg_graph_components_device", "mdbg_graph_contigs", "mdbg_graph_contigs_device", "mdbg_kept_reads", "mdbg_contigs_ms", "mdbg_graph_node_seqs", "mdbg_graph_node_seqs_device", "mdbg_node_seqs_ms", "mdbg_graph_read_paths", "mdbg_graph_read_paths_device", "mdbg_read_paths_ms",
           "mdbg_graph_junctions", "mdbg_graph_junctions_device", "mdbg_junctions_ms", "mdbg_graph_transits", "mdbg_graph_transits_device", "mdbg_transits_ms",
           "mdbg_ingest_batch_packed", "mdbg_ingest_batch_packed_device", "mdbg_sketch_packed_device", "mdbg_pack_device", "mdbg_query_batch", "mdbg_owner_lists", "mdbg_sketch_commit_listed", "mdbg_mark", "mdbg_rewind", "mdbg_set_lmer_filter",
           "mdbg_release_cached_memory", "mdbg_host_alloc", "mdbg_host_free", "mdbg_host_is_pinned", "mdbg_dbg_segments_ms",
           "mdbg_guard_check", "mdbg_guard_report", "mdbg_guard_selftest"]


def lib_path():
    return os.path.join(_HERE, "libmdbg_hip.so")


def load_library():
    """Loads libmdbg_hip.so.  No fallback: a missing library is an error (build with __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError("libmdbg_hip.so not built (%s); run `make -C rust_mdbg_amd/csrc`" % p)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; if this library (linked against
    # /opt/rocm's) is loaded first, a later `import torch` finds no GPU.  Loading torch first makes both share torch's
    # copy (same SONAME).  Plumbing only - nothing of torch is used here.  MDBG_NO_TORCH_PRELOAD=1 disables it.
    import sys
    if "torch" not in sys.modules and not os.environ.get("MDBG_NO_TORCH_PRELOAD"):
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    L = C.CDLL(p)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.mdbg_abi_version.restype = u32
    L.mdbg_build_flags.restype = u32
    L.mdbg_release_cached_memory.restype = u64
    L.mdbg_host_alloc.restype = vp
    L.mdbg_host_alloc.argtypes = [C.c_size_t]
    L.mdbg_host_free.restype = None
    L.mdbg_host_free.argtypes = [vp]
    L.mdbg_host_is_pinned.argtypes = [vp]
    L.mdbg_guard_check.restype = u64
    L.mdbg_guard_check.argtypes = [C.POINTER(u64), C.POINTER(u64)]
    L.mdbg_guard_report.restype = C.c_char_p
    L.mdbg_guard_selftest.restype = C.c_int
    L.mdbg_create.restype = vp
    L.mdbg_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_int)]
    L.mdbg_destroy.restype = None
    L.mdbg_destroy.argtypes = [vp]
    L.mdbg_ingest_batch.argtypes = [vp, vp, vp, u64, u64]
    L.mdbg_ingest_batch_device.argtypes = [vp, vp, vp, u64, u64, u64]
    L.mdbg_sketch_device.argtypes = [vp, vp, vp, u64, u64, u64]
    L.mdbg_insert_resident.argtypes = [vp]
    L.mdbg_ingest_batch_packed.argtypes = [vp, C.POINTER(PackedBatch), u64]
    L.mdbg_ingest_batch_packed_device.argtypes = [vp, C.POINTER(PackedBatch), u64, u64]
    L.mdbg_sketch_packed_device.argtypes = [vp, C.POINTER(PackedBatch), u64, u64]
    L.mdbg_pack_device.argtypes = [vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.mdbg_query_batch.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(u32)), C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
    L.mdbg_query_batch.restype = C.c_int
    L.mdbg_sketch_only.argtypes = [vp, vp, vp, u64, C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
    L.mdbg_finalize.argtypes = [vp, C.POINTER(Nodes)]
    L.mdbg_finalize_device.argtypes = [vp, C.POINTER(Nodes)]
    L.mdbg_finalize_gfa.argtypes = [vp, C.POINTER(Nodes)]
    L.mdbg_set_timing.argtypes = [vp, u32]
    L.mdbg_nodes_digest.argtypes = [vp, C.POINTER(Nodes), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mdbg_reset.argtypes = [vp, u32]
    L.mdbg_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.mdbg_strerror.restype = C.c_char_p
    L.mdbg_strerror.argtypes = [C.c_int]
    L.mdbg_last_error.restype = C.c_char_p
    L.mdbg_last_error.argtypes = [vp]
    L.mdbg_route_pack.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64)]
    L.mdbg_routed_export.argtypes = [vp, u32, vp, vp, u32, C.POINTER(RoutedLists)]
    L.mdbg_resolve_first.argtypes = [vp, vp, vp, u64, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.mdbg_resolve_meta.argtypes = [vp, vp, u64, vp]
    L.mdbg_routed_keys.argtypes = [vp, vp, u64, vp]
    L.mdbg_arena_reserve.argtypes = [vp, u64, C.POINTER(vp)]
    L.mdbg_set_partition.argtypes = [vp, u32, u32]
    L.mdbg_sketch_view.argtypes = [vp, C.POINTER(SketchStore)]
    L.mdbg_ingest_sketch.argtypes = [vp, vp, vp, vp, u64, u64]
    L.mdbg_store_reserve.argtypes = [vp, u64, u64]
    L.mdbg_sketch_reserve.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.mdbg_sketch_commit.argtypes = [vp, u64, u64, vp, u64, u64, u64]
    L.mdbg_owner_counts.argtypes = [vp, u32, vp]
    L.mdbg_owner_lists.argtypes = [vp, u32, vp, C.POINTER(vp)]
    L.mdbg_owner_lists.restype = C.c_int
    L.mdbg_sketch_commit_listed.argtypes = [vp, u64, u64, vp, u64, u64, vp, u64]
    L.mdbg_sketch_commit_listed.restype = C.c_int
    L.mdbg_set_lmer_filter.argtypes = [vp, vp, u64]
    L.mdbg_set_lmer_filter.restype = C.c_int
    L.mdbg_mark.argtypes = [vp, C.POINTER(u64)]
    L.mdbg_mark.restype = C.c_int
    L.mdbg_rewind.argtypes = [vp, u64]
    L.mdbg_rewind.restype = C.c_int
    L.mdbg_last_batch.argtypes = [vp, C.POINTER(BatchInfo)]
    L.mdbg_graph_edges.argtypes = [vp, C.c_float, C.POINTER(EdgeList)]
    L.mdbg_graph_edges_device.argtypes = [vp, C.c_float, C.POINTER(EdgeList)]
    L.mdbg_graph_unitigs.argtypes = [vp, C.POINTER(UnitigList)]
    L.mdbg_graph_unitigs_device.argtypes = [vp, C.POINTER(UnitigList)]
    L.mdbg_graph_simplify.argtypes = [vp, C.POINTER(SimplifyStep), u32, C.POINTER(UnitigList), C.POINTER(SimplifyStats)]
    L.mdbg_graph_simplify_device.argtypes = [vp, C.POINTER(SimplifyStep), u32, C.POINTER(UnitigList), C.POINTER(SimplifyStats)]
    L.mdbg_graph_components.argtypes = [vp, C.POINTER(ComponentList)]
    L.mdbg_graph_components_device.argtypes = [vp, C.POINTER(ComponentList)]
    L.mdbg_graph_contigs.argtypes = [vp, u64, C.POINTER(ContigSeqs)]
    L.mdbg_graph_contigs_device.argtypes = [vp, u64, C.POINTER(ContigSeqs)]
    L.mdbg_kept_reads.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.mdbg_contigs_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_graph_node_seqs.argtypes = [vp, u64, u64, u64, C.POINTER(NodeSeqs)]
    L.mdbg_graph_node_seqs_device.argtypes = [vp, u64, u64, u64, C.POINTER(NodeSeqs)]
    L.mdbg_node_seqs_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_graph_read_paths.argtypes = [vp, u64, u64, C.POINTER(ReadPathList)]
    L.mdbg_graph_read_paths_device.argtypes = [vp, u64, u64, C.POINTER(ReadPathList)]
    L.mdbg_read_paths_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_simplify_edges_removed.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    L.mdbg_graph_junctions.argtypes = [vp, u64, u64, C.POINTER(JunctionList)]
    L.mdbg_graph_junctions_device.argtypes = [vp, u64, u64, C.POINTER(JunctionList)]
    L.mdbg_junctions_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_graph_transits.argtypes = [vp, u64, u64, u64, C.POINTER(TransitList)]
    L.mdbg_graph_transits_device.argtypes = [vp, u64, u64, u64, C.POINTER(TransitList)]
    L.mdbg_transits_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_finalize_begin.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.mdbg_finalize_end.argtypes = [vp, C.POINTER(Nodes), C.POINTER(vp), C.POINTER(u64)]
    L.mdbg_insert_records.argtypes = [vp, vp, u64]
    L.mdbg_sync.argtypes = [vp]
    L.mdbg_copy_to_host.argtypes = [vp, vp, vp, u64]
    L.mdbg_copy_to_device.argtypes = [vp, vp, vp, u64]
    L.mdbg_synth_reads_device.argtypes = [vp, C.POINTER(SynthParams), u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    for f in ("mdbg_ingest_batch", "mdbg_ingest_batch_device", "mdbg_sketch_device", "mdbg_insert_resident", "mdbg_sketch_only",
              "mdbg_finalize", "mdbg_finalize_device", "mdbg_reset", "mdbg_get_stats", "mdbg_route_pack", "mdbg_insert_records", "mdbg_sync",
              "mdbg_synth_reads_device", "mdbg_copy_to_host", "mdbg_copy_to_device", "mdbg_routed_export", "mdbg_resolve_first",
              "mdbg_resolve_meta", "mdbg_routed_keys", "mdbg_arena_reserve", "mdbg_set_partition", "mdbg_sketch_view",
              "mdbg_ingest_sketch", "mdbg_finalize_begin", "mdbg_finalize_end", "mdbg_ingest_batch_packed",
              "mdbg_ingest_batch_packed_device", "mdbg_sketch_packed_device", "mdbg_pack_device"):
        getattr(L, f).restype = C.c_int
    _align.declare_hip(L)                                  # include/mdbg_align.h
    _chains.declare_hip(L)                                 # include/mdbg_chain.h
    _LIB = L
    return L


def release_cached_memory():
    """hands the device blocks the library keeps for reuse back to the runtime; returns the number of bytes released (include/mdbg_hip.h)"""
    n = int(load_library().mdbg_release_cached_memory())
    guard_check()
    return n


# MDBG_GUARD (test hook, include/mdbg_hip.h): every device block lies between two bands that nobody may write.  With it in the environment at import every library call
# of a context is followed by a check of all bands, so that a damaged band is pinned to the call that did it, not to a later free.  GUARD_SEEN: checks made, and the most
# live blocks / payload bytes one of them looked at (tests/test_gpu_guard.py prints them: a run that checked nothing must not pass).
GUARD = "MDBG_GUARD" in os.environ
GUARD_SEEN = {"calls": 0, "blocks": 0, "bytes": 0, "violations": 0}


def guard_check():
    """no-op unless MDBG_GUARD was set at import; AssertionError(report) as soon as a band is damaged"""
    if not GUARD:
        return
    L = load_library()
    nb, by = C.c_uint64(0), C.c_uint64(0)
    bad = L.mdbg_guard_check(C.byref(nb), C.byref(by))
    GUARD_SEEN["calls"] += 1
    GUARD_SEEN["blocks"] = max(GUARD_SEEN["blocks"], int(nb.value))
    GUARD_SEEN["bytes"] = max(GUARD_SEEN["bytes"], int(by.value))
    if bad > GUARD_SEEN["violations"]:         # (the count never goes down: what has been raised once is not raised again by the calls that follow, a close() on the way out among them)
        GUARD_SEEN["violations"] = int(bad)
        raise AssertionError("MDBG_GUARD: %d damaged band(s); first: %s" % (bad, L.mdbg_guard_report().decode()))


def _np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


def edge_columns(e):
    """the five arrays of an EdgeList with HOST pointers (a unitig list's `edges`), copied -> dict by field name"""
    return {f: _np(getattr(e, f), int(e.n), t) for f, t in EDGE_FIELDS}


def concat_reads(reads):
    """list[bytes] -> (uint8 bases, uint64 offsets[n+1]) — the batch layout of mdbg_ingest_batch"""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if reads else np.zeros(0, np.uint8)
    return bases, offs


class Mdbg:
    """One context = one device-resident sketch store + k-min-mer table (dbg_nodes, src/main.rs:595)."""

    def __init__(self, k, l, density, min_abundance=2, reads_already_hpc=False, device=-1, flags=0, table_capacity_hint=0, syncmer_s=None, keep_reads=False,
                 prefilter=False, prefilter_cells=0):
        """keep_reads: the context keeps every batch it ingests with bases, packed 2 bits per base, on the device (MDBG_FLAG_KEEP_READS): graph_contigs()
        prefilter: the counting pre-filter (MDBG_FLAG_PREFILTER, needs min_abundance >= 2): a k-min-mer enters the table only when its filter cell has been hit twice;
        prefilter_cells: number of 2-bit cells, 0 = 2^32"""
        self.L = load_library()
        if keep_reads:
            flags |= FLAG_KEEP_READS
        if prefilter:
            flags |= FLAG_PREFILTER
        self.params = Params(k=k, l=l, density=density, min_abundance=min_abundance, reads_already_hpc=int(reads_already_hpc),
                             device=device, flags=flags, table_capacity_hint=table_capacity_hint,
                             scheme=0 if syncmer_s is None else 1, syncmer_s=0 if syncmer_s is None else syncmer_s,        # syncmer_s: --syncmers -s
                             prefilter_cells=prefilter_cells)
        err = C.c_int(0)
        self.h = self.L.mdbg_create(C.byref(self.params), C.byref(err))
        if not self.h:
            raise MdbgError(err.value, self.L.mdbg_strerror(err.value).decode())
        self.k = k

    def _chk(self, e):
        guard_check()
        if e != 0:
            raise MdbgError(e, (self.L.mdbg_last_error(self.h) or self.L.mdbg_strerror(e)).decode())

    # --- process_read_aux over a batch (host buffers) ---
    def ingest(self, bases, offsets, first_read_ordinal=0):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(self.L.mdbg_ingest_batch(self.h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, first_read_ordinal))

    def ingest_reads(self, reads, first_read_ordinal=0):
        b, o = concat_reads(reads)
        self.ingest(b, o, first_read_ordinal)

    # --- device-resident buffers (raw pointers, e.g. torch.Tensor.data_ptr()) ---
    def ingest_device(self, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal=0):
        self._chk(self.L.mdbg_ingest_batch_device(self.h, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal))

    def sketch_device(self, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal=0):
        self._chk(self.L.mdbg_sketch_device(self.h, d_bases, d_offsets, n_reads, n_bases, first_read_ordinal))

    def insert_resident(self):
        self._chk(self.L.mdbg_insert_resident(self.h))

    # --- 2-bit packed input (mdbg_packed_batch) ---
    def ingest_packed(self, packed, first_read_ordinal=0):
        """packed: dict from rust_mdbg_amd.emit.pack_reads (host arrays words / offsets / exc_pos / exc_val)"""
        b = PackedBatch(packed["words"].ctypes.data, packed["offsets"].ctypes.data, len(packed["offsets"]) - 1,
                        packed["exc_pos"].ctypes.data, packed["exc_val"].ctypes.data, len(packed["exc_pos"]))
        self._chk(self.L.mdbg_ingest_batch_packed(self.h, C.byref(b), first_read_ordinal))

    def ingest_packed_device(self, d_words, d_offsets, n_reads, n_bases, first_read_ordinal=0, d_exc_pos=0, d_exc_val=0, n_exc=0, sketch_only=False):
        b = PackedBatch(d_words, d_offsets, n_reads, d_exc_pos, d_exc_val, n_exc)
        fn = self.L.mdbg_sketch_packed_device if sketch_only else self.L.mdbg_ingest_batch_packed_device
        self._chk(fn(self.h, C.byref(b), n_bases, first_read_ordinal))

    def pack_device(self, d_bases, n_bases, d_words, d_exc_pos=0, d_exc_val=0, exc_cap=0):
        n = C.c_uint64()
        self._chk(self.L.mdbg_pack_device(self.h, d_bases, n_bases, d_words, d_exc_pos, d_exc_val, exc_cap, C.byref(n)))
        return n.value

    def query(self, bases, offsets):
        """--read_stats: (counts u32[n_windows], per-read offsets u64[n_reads + 1])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        pc, po, nw = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint64()
        self._chk(self.L.mdbg_query_batch(self.h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(pc), C.byref(po), C.byref(nw)))
        return _np(pc, nw.value, np.uint32), _np(po, n + 1, np.uint64)

    def store_sketch(self):
        """host copy of the whole resident sketch store: hashes, positions, per-read offsets"""
        v = self.sketch_view()
        m, n = int(v.n_minimizers), int(v.n_reads)
        return dict(hashes=self.to_host(v.d_hashes, m * 8, np.uint64) if m else np.zeros(0, np.uint64),
                    pos=self.to_host(v.d_positions, m * 4, np.uint32).astype(np.uint64) if m else np.zeros(0, np.uint64),
                    off=self.to_host(v.d_read_offsets, (n + 1) * 8, np.uint64))

    # --- Read::extract seam ---
    def sketch(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        ph, pp, po = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        m = C.c_uint64()
        self._chk(self.L.mdbg_sketch_only(self.h, bases.ctypes.data, offsets.ctypes.data, n, C.byref(ph), C.byref(pp), C.byref(po), C.byref(m)))
        return dict(hashes=_np(ph, m.value, np.uint64), pos=_np(pp, m.value, np.uint64), off=_np(po, n + 1, np.uint64))

    def finalize(self, gfa_only=False):
        """-> the node table as numpy arrays.  gfa_only: the table stays on the device (where mdbg_graph_edges reads it) and only what the S lines of a .gfa
        print (index, length, abundance: 10 bytes per node instead of 8 k + 58) is copied to the host; the other entries are None"""
        nd = Nodes()
        if gfa_only:
            self._chk(self.L.mdbg_finalize_gfa(self.h, C.byref(nd)))
            n = self._table_rows = int(nd.n)
            return dict(n_nodes=n, n_nodes_before=int(nd.n_distinct), n_wrapped=int(nd.n_wrapped), k=int(nd.k), keys=None, index=_np(nd.index, n, np.uint32),
                        abundance=_np(nd.abundance, n, np.uint16), seqlen=_np(nd.seqlen, n, np.uint32), shift=None, shift_full=None, src_read=None, src_start=None,
                        src_end=None, reversed=None)
        self._chk(self.L.mdbg_finalize(self.h, C.byref(nd)))
        n, k = nd.n, nd.k
        self._table_rows = int(n)
        return dict(n_nodes=int(n), n_nodes_before=int(nd.n_distinct), n_wrapped=int(nd.n_wrapped),
                    keys=_np(nd.keys, n * k, np.uint64).reshape(n, k), index=_np(nd.index, n, np.uint32),
                    abundance=_np(nd.abundance, n, np.uint16), seqlen=_np(nd.seqlen, n, np.uint32),
                    shift=_np(nd.shift, 2 * n, np.uint16).reshape(n, 2), shift_full=_np(nd.shift_full, 2 * n, np.uint64).reshape(n, 2),
                    src_read=_np(nd.src_read, n, np.uint64), src_start=_np(nd.src_start, n, np.uint64),
                    src_end=_np(nd.src_end, n, np.uint64), reversed=_np(nd.reversed, n, np.uint8))

    def finalize_device(self):
        """node table left in device memory; returns the raw mdbg_nodes struct (device pointers)"""
        nd = Nodes()
        self._chk(self.L.mdbg_finalize_device(self.h, C.byref(nd)))
        self._table_rows = int(nd.n)
        return nd

    def set_timing(self, level):
        """0: no HIP events, 1: around the tile kernel only, 2 (default): also around the stages (include/mdbg_hip.h, mdbg_set_timing)"""
        self._chk(self.L.mdbg_set_timing(self.h, level))

    def nodes_digest(self, nd):
        """(sum, xor) over the rows of a DEVICE node table (finalize_device / DistMdbg.finalize): the order-free digest of {(key, abundance)}, include/mdbg_hip.h"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mdbg_nodes_digest(self.h, C.byref(nd), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def reset(self, new_k):
        self._chk(self.L.mdbg_reset(self.h, new_k))
        if new_k:
            self.k = new_k

    def set_lmer_filter(self, codes):
        """--lmer-counts: codes = uint64 array of the selected l-mers' 2-bit codes, both orientations (emit.lmer_filter_from_counts);
        None switches the filter off.  Before the first batch."""
        if codes is None:
            self._chk(self.L.mdbg_set_lmer_filter(self.h, None, 0))
            return
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        keep = codes if len(codes) else np.zeros(1, dtype=np.uint64)        # a non-null pointer also for the empty selection
        self._chk(self.L.mdbg_set_lmer_filter(self.h, keep.ctypes.data, len(codes)))

    def mark(self):
        """-> token naming what is resident now (see rewind)"""
        mk = C.c_uint64()
        self._chk(self.L.mdbg_mark(self.h, C.byref(mk)))
        return int(mk.value)

    def rewind(self, mark):
        """forget every batch ingested after mark() and clear the node table; follow with reset(k) to re-window what is left"""
        self._chk(self.L.mdbg_rewind(self.h, mark))

    # --- multi-GPU stage calls (raw device pointers; see rust_mdbg_amd/dist.py for the driver) ---
    def route_pack(self, world):
        """-> (device pointer to bucketed records of k+2 u64, [records per destination])"""
        ptr = C.c_void_p()
        counts = (C.c_uint64 * 64)()
        self._chk(self.L.mdbg_route_pack(self.h, world, C.byref(ptr), counts))
        return ptr.value or 0, [int(counts[i]) for i in range(world)]

    def arena_reserve(self, n):
        """-> device pointer where n more routed records (k+2 u64 each) may be received in place"""
        ptr = C.c_void_p()
        self._chk(self.L.mdbg_arena_reserve(self.h, n, C.byref(ptr)))
        return ptr.value or 0

    def insert_records(self, d_records, n):
        self._chk(self.L.mdbg_insert_records(self.h, d_records, n))

    def routed_export(self, world, span_lo, span_rank):
        """owner side: the two query lists bucketed by answering rank -> RoutedLists (device pointers + host counts)"""
        lo = np.ascontiguousarray(span_lo, dtype=np.uint64)
        rk = np.ascontiguousarray(span_rank, dtype=np.uint32)
        out = RoutedLists()
        self._chk(self.L.mdbg_routed_export(self.h, world, lo.ctypes.data, rk.ctypes.data, len(lo), C.byref(out)))
        return out

    def resolve_first(self, d_ord, d_solid, n, d_rank_first, d_rank_solid):
        tf, ts = C.c_uint64(), C.c_uint64()
        self._chk(self.L.mdbg_resolve_first(self.h, d_ord, d_solid, n, d_rank_first, d_rank_solid, C.byref(tf), C.byref(ts)))
        return tf.value, ts.value

    def resolve_meta(self, d_ord, n, d_meta):
        self._chk(self.L.mdbg_resolve_meta(self.h, d_ord, n, d_meta))

    def routed_keys(self, d_slot, n, d_keys):
        self._chk(self.L.mdbg_routed_keys(self.h, d_slot, n, d_keys))

    # --- replicated-sketch multi-GPU mode ---
    def set_partition(self, world, rank):
        self._chk(self.L.mdbg_set_partition(self.h, world, rank))

    def sketch_view(self):
        s = SketchStore()
        self._chk(self.L.mdbg_sketch_view(self.h, C.byref(s)))
        return s

    def ingest_sketch(self, d_hashes, d_positions, d_read_offsets, n_reads, first_read_ordinal):
        self._chk(self.L.mdbg_ingest_sketch(self.h, d_hashes, d_positions, d_read_offsets, n_reads, first_read_ordinal))

    def graph_edges(self, presimp=0.01, raw=False):
        """edges of the node table of the last finalize(), built on the GPU (src/main.rs:1017-1117)
        -> dict(n1, o1, n2, o2, overlap, presimp_removed) of numpy arrays, o1/o2 as ASCII '+' / '-'; raw=True: the C struct"""
        e = EdgeList()
        self._chk(self.L.mdbg_graph_edges(self.h, presimp, C.byref(e)))
        if raw:
            return e
        n = int(e.n)
        g = lambda p, t: np.ctypeslib.as_array(p, shape=(n,)).astype(t, copy=True) if n else np.zeros(0, t)
        return dict(n1=g(e.n1, np.uint32), o1=g(e.o1, np.uint8), n2=g(e.n2, np.uint32), o2=g(e.o2, np.uint8), overlap=g(e.overlap, np.uint32),
                    presimp_removed=int(e.presimp_removed))

    def graph_edges_device(self, presimp=0.01):
        """-> EdgeList with DEVICE pointers (valid until the next edge call)"""
        e = EdgeList()
        self._chk(self.L.mdbg_graph_edges_device(self.h, presimp, C.byref(e)))
        return e

    def graph_unitigs(self, raw=False):
        """unitigs of the last finalize() + graph_edges() and their base-space copy plan, compacted on the GPU (`gfatools asm -u` + the planning half of
        src/to_basespace.rs; no tip / bubble removal: that is graph_simplify; single GPU) -> dict of numpy arrays named like the fields of mdbg_unitig_list (include/mdbg_hip.h), with
        `edges` a dict like graph_edges() whose n1 / n2 are 0-based unitig numbers; raw=True: the C struct with HOST arrays (for Emitter.contigs)"""
        u = UnitigList()
        self._chk(self.L.mdbg_graph_unitigs(self.h, C.byref(u)))
        return u if raw else self._unitig_dict(u)

    @staticmethod
    def _unitig_dict(u):
        cnt = unitig_counts(u)
        out = {f: _np(getattr(u, f), cnt[f], t) for f, t in UNITIG_FIELDS}
        if not len(out["offsets"]):
            out["offsets"] = np.zeros(1, np.uint64)
        out.update(n_unitigs=int(u.n_unitigs), n_entries=int(u.n_entries), n_rounds=int(u.n_rounds), edges=edge_columns(u.edges))
        return out

    def graph_unitigs_device(self):
        """-> UnitigList with DEVICE pointers (valid until the next unitig / edge / finalize / reset call)"""
        u = UnitigList()
        self._chk(self.L.mdbg_graph_unitigs_device(self.h, C.byref(u)))
        return u

    def _simplify_stats(self, st, steps, n_entries):
        """entries_copied: the entries the REPEATS and NESTED steps added, from n_entries == rows of the node table - total_nodes_removed + all copies of the
        schedule; 0 for a schedule without such a step, None if this object has not seen the finalize call that made the table"""
        n = int(st.n_steps)
        per_step, total = C.POINTER(C.c_uint64)(), C.c_uint64()
        self._chk(self.L.mdbg_simplify_edges_removed(self.h, C.byref(per_step), C.byref(total)))
        return dict(unitigs_removed=[int(st.unitigs_removed[i]) for i in range(n)], nodes_removed=[int(st.nodes_removed[i]) for i in range(n)],
                    edges_removed=[int(per_step[i]) for i in range(n)], total_unitigs_removed=int(st.total_unitigs_removed),
                    total_nodes_removed=int(st.total_nodes_removed), total_edges_removed=int(total.value), n_compactions=int(st.n_compactions),
                    n_rounds_total=int(st.n_rounds_total), n_syncs=int(st.n_syncs), entries_copied=self._entries_copied(steps, int(n_entries), int(st.total_nodes_removed)))

    def _entries_copied(self, steps, n_entries, total_nodes_removed):
        if not any(int(s[0]) in (MDBG_SIMPLIFY_REPEATS, MDBG_SIMPLIFY_NESTED) for s in steps) or n_entries == 0:
            return 0
        rows = getattr(self, "_table_rows", None)
        return None if rows is None else n_entries - (rows - total_nodes_removed)

    def graph_simplify(self, steps, raw=False):
        """the unitigs that are left after a schedule of tip, simple-bubble, small-component and edge-pruning steps, decided and compacted on the GPU (mdbg_graph_simplify, include/mdbg_hip.h: this
        project's own order-free rules in the spirit of `gfatools asm -t N,L -b L`, NOT bit-parity with gfatools).  steps: [(kind, max_nodes, max_bases)], e.g.
        MAGIC_SIMPLIFY_STEPS; an empty schedule gives graph_unitigs().  -> the dict of graph_unitigs() plus `stats` (per step: unitigs / nodes / edge records removed; totals);
        raw=True: (the C struct with HOST arrays, stats)"""
        arr, n = simplify_steps(steps)
        u, st = UnitigList(), SimplifyStats()
        self._chk(self.L.mdbg_graph_simplify(self.h, arr, n, C.byref(u), C.byref(st)))
        stats = self._simplify_stats(st, steps, u.n_entries)
        if raw:
            return u, stats
        return dict(self._unitig_dict(u), stats=stats)

    def graph_simplify_device(self, steps):
        """-> (UnitigList with DEVICE pointers, valid until the next unitig / simplify / edge / finalize / reset call; stats)"""
        arr, n = simplify_steps(steps)
        u, st = UnitigList(), SimplifyStats()
        self._chk(self.L.mdbg_graph_simplify_device(self.h, arr, n, C.byref(u), C.byref(st)))
        return u, self._simplify_stats(st, steps, u.n_entries)

    def graph_components(self):
        """connected components of the current unitig list (the last graph_unitigs* / graph_simplify* call), found on the GPU: two unitigs are joined iff an edge of
        the list names both (mdbg_graph_components, include/mdbg_hip.h); components are numbered by their smallest unitig.  Leaves the list as it is.
        -> dict(n_unitigs, n_components, component u32[n_unitigs], and per component first_unitig, unitigs, nodes, bases, kc_sum, circular)"""
        cl = ComponentList()
        self._chk(self.L.mdbg_graph_components(self.h, C.byref(cl)))
        nu, nc = int(cl.n_unitigs), int(cl.n_components)
        return dict({f: _np(getattr(cl, f), nu if per_unitig else nc, t) for f, t, per_unitig in COMPONENT_FIELDS}, n_unitigs=nu, n_components=nc)

    def graph_components_device(self):
        """-> ComponentList with DEVICE pointers (valid until the next component call, a simplify call with a component step, or a call that ends the unitig list)"""
        cl = ComponentList()
        self._chk(self.L.mdbg_graph_components_device(self.h, C.byref(cl)))
        return cl

    def graph_read_paths(self, first_read=0, max_reads=0):
        """the resident reads [first_read, first_read + max_reads) (0: to the end; slot order) threaded through the current unitig list (the last graph_unitigs* /
        graph_simplify* call) on the GPU: which unitigs, in which order and orientation, each read walks (mdbg_graph_read_paths, include/mdbg_hip.h).  Leaves the list
        as it is.  -> dict(first_read, n_reads, n_windows, n_placed, n_steps, n_unitigs; per read ordinal, read_windows, step_offsets[n_reads + 1]; per step first_window,
        step_windows, unitig, first_entry, strand; per unitig support_windows, support_steps)"""
        rp = ReadPathList()
        self._chk(self.L.mdbg_graph_read_paths(self.h, first_read, max_reads, C.byref(rp)))
        n = dict(read=int(rp.n_reads), step=int(rp.n_steps), unitig=int(rp.n_unitigs))
        out = {f: _np(getattr(rp, f), n[per], t) for f, t, per in READ_PATH_FIELDS}
        out["step_offsets"] = _np(rp.step_offsets, n["read"] + 1, np.uint64) if rp.step_offsets else np.zeros(1, np.uint64)
        out.update(first_read=int(rp.first_read), n_reads=n["read"], n_windows=int(rp.n_windows), n_placed=int(rp.n_placed), n_steps=n["step"], n_unitigs=n["unitig"])
        return out

    def graph_read_paths_device(self, first_read=0, max_reads=0):
        """-> ReadPathList with DEVICE pointers (valid until the next read-path call)"""
        rp = ReadPathList()
        self._chk(self.L.mdbg_graph_read_paths_device(self.h, first_read, max_reads, C.byref(rp)))
        return rp

    def read_paths_ms(self):
        """device time of the last graph_read_paths* call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_read_paths_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def graph_junctions(self, first_read=0, max_reads=0):
        """read support per junction of the current unitig list, counted on the GPU over the resident reads [first_read, first_read + max_reads) (0: to the end): how
        many reads cross each edge record, and where reads cross without a record (mdbg_graph_junctions, include/mdbg_hip.h).  Leaves the list and every other result
        as they are.  -> dict(first_read, n_reads, n_adjacent, n_links, n_crossings, n_explained, n_missing_crossings, n_records, n_missing; per edge record support;
        per missing key missing_unitig1, missing_entry1, missing_strand1, missing_unitig2, missing_entry2, missing_strand2, missing_count)"""
        jl = JunctionList()
        self._chk(self.L.mdbg_graph_junctions(self.h, first_read, max_reads, C.byref(jl)))
        n = dict(record=int(jl.n_records), missing=int(jl.n_missing))
        out = {f: _np(getattr(jl, f), n[per], t) for f, t, per in JUNCTION_FIELDS}
        out.update({f: int(getattr(jl, f)) for f in JUNCTION_COUNTS}, first_read=int(jl.first_read), n_records=n["record"], n_missing=n["missing"])
        return out

    def graph_junctions_device(self, first_read=0, max_reads=0):
        """-> JunctionList with DEVICE pointers (valid until the next junction call)"""
        jl = JunctionList()
        self._chk(self.L.mdbg_graph_junctions_device(self.h, first_read, max_reads, C.byref(jl)))
        return jl

    def junctions_ms(self):
        """device time of the last graph_junctions* call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_junctions_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def graph_transits(self, first_read=0, max_reads=0, min_support=1):
        """the reads that span a unitig of the current list end to end, found on the GPU over the resident reads [first_read, first_read + max_reads) (0: to the end):
        per (entrance, exit) pair the reads take through a unitig its count, and per unitig whether the pairs seen min_support times or more match its entrances to
        its exits one to one (mdbg_graph_transits, include/mdbg_hip.h).  Leaves the list and every other result as they are.
        -> dict(first_read, n_reads, n_crossings, n_explained, n_passes, n_transits, n_unitigs, n_repeats, n_resolved; per transit key unitig, in_unitig, in_entry,
        in_strand, out_unitig, out_entry, out_strand, in_record, out_record, count; per unitig n_in, n_out, passes, verdict)"""
        tl = TransitList()
        self._chk(self.L.mdbg_graph_transits(self.h, first_read, max_reads, min_support, C.byref(tl)))
        n = dict(transit=int(tl.n_transits), unitig=int(tl.n_unitigs))
        out = {f: _np(getattr(tl, f), n[per], t) for f, t, per in TRANSIT_FIELDS}
        out.update({f: int(getattr(tl, f)) for f in TRANSIT_COUNTS + ("n_repeats", "n_resolved")}, first_read=int(tl.first_read), n_transits=n["transit"], n_unitigs=n["unitig"])
        return out

    def graph_transits_device(self, first_read=0, max_reads=0, min_support=1):
        """-> TransitList with DEVICE pointers (valid until the next transit call)"""
        tl = TransitList()
        self._chk(self.L.mdbg_graph_transits_device(self.h, first_read, max_reads, min_support, C.byref(tl)))
        return tl

    def transits_ms(self):
        """device time of the last graph_transits* call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_transits_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def graph_alignments(self, first_read=0, max_reads=0):
        """the resident reads [first_read, first_read + max_reads) (0: to the end) aligned to the current unitig list on the GPU: the steps of graph_read_paths chained
        over the list's edge records into alignments, with base coordinates on the read and on the path of unitigs (mdbg_graph_alignments, include/mdbg_align.h).  The
        call is the read-path call of the range too; it leaves the list and every other result as they are.
        -> dict(first_read, n_reads, n_windows, n_placed, n_steps, n_chained, n_alignments, n_wraps, n_unitigs; per read ordinal, read_windows, step_offsets[n_reads + 1],
        aln_offsets[n_reads + 1]; per step first_window, step_windows, unitig, first_entry, strand, step_record; aln_step_offsets[n_alignments + 1]; per alignment
        aln_windows, query_begin, query_end, path_length, path_begin, path_end)"""
        al = _align.AlignmentList()
        self._chk(self.L.mdbg_graph_alignments(self.h, first_read, max_reads, C.byref(al)))
        return _align.alignment_dict(al)

    def graph_alignments_device(self, first_read=0, max_reads=0):
        """-> AlignmentList with DEVICE pointers (valid until the next alignment call; its step columns until the next read-path call)"""
        al = _align.AlignmentList()
        self._chk(self.L.mdbg_graph_alignments_device(self.h, first_read, max_reads, C.byref(al)))
        return al

    def alignments_ms(self):
        """device time of the last graph_alignments* / align_batch call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_alignments_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def align_batch(self, bases, offsets):
        """sequences that are NOT resident (genes, a reference, contigs) aligned to the current unitig list: the batch is sketched behind the store, aligned as
        graph_alignments aligns resident reads, and the store rolled back; nothing but the alignment and the read-path result changes (mdbg_graph_align_batch,
        include/mdbg_align.h).  -> the dict of graph_alignments; read q is query q, ordinal[q] == q"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        al = _align.AlignmentList()
        self._chk(self.L.mdbg_graph_align_batch(self.h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, C.byref(al)))
        return _align.alignment_dict(al)

    def graph_chains(self, first_read=0, max_reads=0, max_skew=0, max_gap=0):
        """graph_alignments over the same range, and consecutive alignments of a read joined where the graph bridges the unplaced windows between them: inside one
        unitig or over one edge record, with the entries of the bridge at most max_skew away from the windows of the gap and the gap at most max_gap windows
        (0: no limit) (mdbg_graph_chains, include/mdbg_chain.h).  -> dict(n_bridges, n_bridges_inside, n_bridges_record, n_chains, n_gap_windows; per alignment
        bridge_record, bridge_entries; chain_offsets[n_reads + 1], chain_aln_offsets[n_chains + 1]; per chain chain_windows, chain_gap_windows, query_begin,
        query_end, path_length, path_begin, path_end; alignments = the dict of graph_alignments)"""
        ch = _chains.ChainList()
        self._chk(self.L.mdbg_graph_chains(self.h, first_read, max_reads, max_skew, max_gap, C.byref(ch)))
        return _chains.chain_dict(ch)

    def graph_chains_device(self, first_read=0, max_reads=0, max_skew=0, max_gap=0):
        """-> ChainList with DEVICE pointers (valid until the next chain call; its alignment columns until the next alignment call)"""
        ch = _chains.ChainList()
        self._chk(self.L.mdbg_graph_chains_device(self.h, first_read, max_reads, max_skew, max_gap, C.byref(ch)))
        return ch

    def chains_ms(self):
        """device time of the last graph_chains* / chain_batch call, the alignment stage inside it included, in milliseconds"""
        ms = C.c_double(0)
        self._chk(self.L.mdbg_chains_ms(self.h, C.byref(ms)))
        return ms.value

    def chain_batch(self, bases, offsets, max_skew=0, max_gap=0):
        """align_batch with the chain stage behind it (mdbg_graph_chain_batch, include/mdbg_chain.h) -> the dict of graph_chains; read q is query q"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ch = _chains.ChainList()
        self._chk(self.L.mdbg_graph_chain_batch(self.h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, max_skew, max_gap, C.byref(ch)))
        return _chains.chain_dict(ch)

    def kept_reads(self):
        """the resident read store of a keep_reads context -> dict(n_reads, n_bases, bytes); bytes = n_bases / 4 + 8 per read + 9 per exception, up to the
        rounding of each batch (include/mdbg_hip.h, mdbg_kept_reads)"""
        r, b, y = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.mdbg_kept_reads(self.h, C.byref(r), C.byref(b), C.byref(y)))
        return dict(n_reads=int(r.value), n_bases=int(b.value), bytes=int(y.value))

    def graph_contigs(self, min_len=0, device=False):
        """the sequences of the current unitig list (the last graph_unitigs* / graph_simplify* call) stitched on the GPU from the kept reads (keep_reads=True),
        byte for byte what Emitter.contigs makes of the same reads on the host; only unitigs of at least min_len bases, in list order.
        -> dict(n_contigs, n_bases, bases u8[n_bases], offsets u64[n_contigs + 1], unitig u64[n_contigs]); device=True: the ContigSeqs struct with DEVICE
        pointers, owned by the context until its next graph_contigs call (they survive rewind / reset / ingest)"""
        cs = ContigSeqs()
        if device:
            self._chk(self.L.mdbg_graph_contigs_device(self.h, min_len, C.byref(cs)))
            return cs
        self._chk(self.L.mdbg_graph_contigs(self.h, min_len, C.byref(cs)))
        n = int(cs.n_contigs)
        return dict(n_contigs=n, n_bases=int(cs.n_bases), bases=_np(cs.bases, int(cs.n_bases), np.uint8), offsets=_np(cs.offsets, n + 1, np.uint64),
                    unitig=_np(cs.unitig, n, np.uint64))

    def contigs_ms(self):
        """device time of the stitch kernel of the last graph_contigs call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_contigs_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def graph_node_seqs(self, first_row=0, max_rows=0, max_bases=0, device=False, raw=False):
        """the sequences of rows [first_row, first_row + n_rows) of the current node table (the last finalize*), gathered on the GPU from the kept reads
        (keep_reads=True): reads[src_read][src_start:src_end], reverse-complemented through utils::revcomp where `reversed` — what a row's .sequences line prints.
        n_rows is the largest count <= max_rows whose sequences together are <= max_bases bytes (0: no limit; at least one row while first_row < n); a loop
        `first_row += n_rows` ends at n_rows == 0.
        -> dict(first_row, n_rows, n_bases, bases u8[n_bases], offsets u64[n_rows + 1]); device=True: the dict holds DEVICE addresses (ints) instead of arrays;
        raw=True: the NodeSeqs struct with HOST arrays, not copied (Emitter.write_sequences_from_kept).  Either way the buffers are the context's until its
        next graph_node_seqs call."""
        ns = NodeSeqs()
        if device:
            self._chk(self.L.mdbg_graph_node_seqs_device(self.h, first_row, max_rows, max_bases, C.byref(ns)))
            return dict(first_row=int(ns.first_row), n_rows=int(ns.n_rows), n_bases=int(ns.n_bases), bases=C.cast(ns.bases, C.c_void_p).value or 0,
                        offsets=C.cast(ns.offsets, C.c_void_p).value or 0)
        self._chk(self.L.mdbg_graph_node_seqs(self.h, first_row, max_rows, max_bases, C.byref(ns)))
        if raw:
            return ns
        n = int(ns.n_rows)
        return dict(first_row=int(ns.first_row), n_rows=n, n_bases=int(ns.n_bases), bases=_np(ns.bases, int(ns.n_bases), np.uint8), offsets=_np(ns.offsets, n + 1, np.uint64))

    def node_seqs_ms(self):
        """device time of the gather kernel of the last graph_node_seqs call, in milliseconds"""
        ms = C.c_double()
        self._chk(self.L.mdbg_node_seqs_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def store_reserve(self, n_minimizers_total, n_reads_total):
        self._chk(self.L.mdbg_store_reserve(self.h, n_minimizers_total, n_reads_total))

    def sketch_reserve(self, n_minimizers):
        """-> (d_hashes, d_positions, region): an uncommitted region at the end of the resident store to receive into"""
        h, p, r = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._chk(self.L.mdbg_sketch_reserve(self.h, n_minimizers, C.byref(h), C.byref(p), C.byref(r)))
        return h.value or 0, p.value or 0, r.value

    def sketch_commit(self, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, owned_windows=None):
        """owned_windows: number of windows of this batch the context owns (from the sender's owner_counts), None = unknown"""
        ow = 0xFFFFFFFFFFFFFFFF if owned_windows is None else int(owned_windows)
        self._chk(self.L.mdbg_sketch_commit(self.h, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, ow))

    def owner_lists(self, world):
        """-> (counts per owning rank, DEVICE pointer to the window lists bucketed by owner; an entry = two uint32: window start, read) for the
        batch registered last"""
        out = (C.c_uint64 * world)()
        p = C.c_void_p()
        self._chk(self.L.mdbg_owner_lists(self.h, world, out, C.byref(p)))
        return [int(x) for x in out], (p.value or 0)

    def sketch_commit_listed(self, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, d_list, n_list):
        self._chk(self.L.mdbg_sketch_commit_listed(self.h, region, n_minimizers, d_read_offsets, n_reads, first_read_ordinal, d_list, n_list))

    def owner_counts(self, world):
        """windows of the batch registered last per owning rank -> list of `world` ints"""
        out = (C.c_uint64 * world)()
        self._chk(self.L.mdbg_owner_counts(self.h, world, out))
        return [int(x) for x in out]

    def last_batch(self):
        b = BatchInfo()
        self._chk(self.L.mdbg_last_batch(self.h, C.byref(b)))
        return b

    def finalize_begin(self):
        """-> (d_bm_first, d_bm_solid, n_words): this rank's bitmaps over the global sketch, to be summed over ranks"""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._chk(self.L.mdbg_finalize_begin(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value or 0, b.value or 0, n.value

    def finalize_end(self):
        """-> (Nodes with device pointers, d_row, n_nodes_global)"""
        nd, row, ng = Nodes(), C.c_void_p(), C.c_uint64()
        self._chk(self.L.mdbg_finalize_end(self.h, C.byref(nd), C.byref(row), C.byref(ng)))
        return nd, row.value or 0, ng.value

    def to_host(self, d_ptr, nbytes, dtype=np.uint8):
        """copy nbytes of device memory into a fresh numpy array"""
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._chk(self.L.mdbg_copy_to_host(self.h, out.ctypes.data, d_ptr, out.nbytes))
        return out

    def sync(self):
        self._chk(self.L.mdbg_sync(self.h))

    def stats(self):
        s = Stats()
        self._chk(self.L.mdbg_get_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in Stats._fields_ if f != "reserved"}

    def synth_reads_device(self, seed, genome_len, n_reads, mean_len=15000, sd_len=1500, min_len=8000, max_len=25000, err_ppm=1000, first_read=0):
        """-> (d_bases ptr, d_offsets ptr, n_bases); buffers are owned by the context (valid until the next call)"""
        sp = SynthParams(seed=seed, genome_len=genome_len, n_reads=n_reads, mean_len=mean_len, sd_len=sd_len, min_len=min_len,
                         max_len=max_len, err_ppm=err_ppm)
        db, do, nb = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._chk(self.L.mdbg_synth_reads_device(self.h, C.byref(sp), first_read, C.byref(db), C.byref(do), C.byref(nb)))
        return db.value, do.value, nb.value

    def close(self):
        if getattr(self, "h", None):
            self.L.mdbg_destroy(self.h)
            self.h = None
            guard_check()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
