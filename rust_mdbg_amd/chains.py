"""ctypes binding of include/mdbg_chain.h — gapped chains: the alignments of one read joined over a bridge, and their GAF lines.

The calls on a context are methods of api.Mdbg (graph_chains, graph_chains_device, chains_ms, chain_batch); this module holds what they share, as align.py does
for include/mdbg_align.h: the struct mirror, the column table, the prototypes (declared once, on the library api.load_library / emit.load_library has loaded)
and the GAF writer."""
import ctypes as C
import os

import numpy as np

from .align import AlignmentList, alignment_dict, alignment_list


class ChainList(C.Structure):          # mdbg_chain_list
    _fields_ = [("alignments", AlignmentList),
                ("n_bridges", C.c_uint64), ("n_bridges_inside", C.c_uint64), ("n_bridges_record", C.c_uint64), ("n_chains", C.c_uint64), ("n_gap_windows", C.c_uint64),
                ("bridge_record", C.POINTER(C.c_uint32)), ("bridge_entries", C.POINTER(C.c_uint64)), ("chain_offsets", C.POINTER(C.c_uint64)),
                ("chain_aln_offsets", C.POINTER(C.c_uint64)), ("chain_windows", C.POINTER(C.c_uint32)), ("chain_gap_windows", C.POINTER(C.c_uint32)),
                ("query_begin", C.POINTER(C.c_uint32)), ("query_end", C.POINTER(C.c_uint32)),
                ("path_length", C.POINTER(C.c_uint64)), ("path_begin", C.POINTER(C.c_uint64)), ("path_end", C.POINTER(C.c_uint64))]


# (field, dtype, what it has one element of: "alignment" or "chain"); the two offset columns have one element more: CHAIN_OFFSETS
CHAIN_FIELDS = (("bridge_record", np.uint32, "alignment"), ("bridge_entries", np.uint64, "alignment"),
                ("chain_windows", np.uint32, "chain"), ("chain_gap_windows", np.uint32, "chain"), ("query_begin", np.uint32, "chain"), ("query_end", np.uint32, "chain"),
                ("path_length", np.uint64, "chain"), ("path_begin", np.uint64, "chain"), ("path_end", np.uint64, "chain"))
CHAIN_OFFSETS = (("chain_offsets", "read"), ("chain_aln_offsets", "chain"))
CHAIN_COUNTS = ("n_bridges", "n_bridges_inside", "n_bridges_record", "n_chains", "n_gap_windows")      # what adds up over the ranges of a partition of the reads
NOT_BRIDGED, INSIDE = 0xFFFFFFFF, 0xFFFFFFFE

HIP_EXPORTS = ["mdbg_graph_chains", "mdbg_graph_chains_device", "mdbg_chains_ms", "mdbg_graph_chain_batch", "mdbg_graph_chain_batch_device"]
EMIT_EXPORTS = ["mdbg_gaf_append_chains"]


def declare_hip(L):
    """the prototypes of include/mdbg_chain.h that libmdbg_hip exports, on the loaded library"""
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.mdbg_graph_chains.argtypes = [vp, u64, u64, u32, u32, C.POINTER(ChainList)]
    L.mdbg_graph_chains_device.argtypes = [vp, u64, u64, u32, u32, C.POINTER(ChainList)]
    L.mdbg_chains_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_graph_chain_batch.argtypes = [vp, vp, vp, u64, u32, u32, C.POINTER(ChainList)]
    L.mdbg_graph_chain_batch_device.argtypes = [vp, vp, vp, u64, u32, u32, C.POINTER(ChainList)]
    for f in HIP_EXPORTS:
        getattr(L, f).restype = C.c_int


def declare_emit(L):
    """the writer of include/mdbg_chain.h that libmdbg_emit exports, on the loaded library"""
    from .api import UnitigList
    L.mdbg_gaf_append_chains.argtypes = [C.c_char_p, C.c_int, C.POINTER(ChainList), C.POINTER(UnitigList), C.c_void_p]
    L.mdbg_gaf_append_chains.restype = C.c_int


def chain_dict(ch):
    """a ChainList with HOST pointers, copied -> dict by field name; the alignment list it holds under "alignments" (the dict of Mdbg.graph_alignments)"""
    from .api import _np
    al = ch.alignments
    n = dict(read=int(al.n_reads), alignment=int(al.n_alignments), chain=int(ch.n_chains))
    out = {f: _np(getattr(ch, f), n[per], t) for f, t, per in CHAIN_FIELDS}
    for f, per in CHAIN_OFFSETS:
        out[f] = _np(getattr(ch, f), n[per] + 1, np.uint64) if getattr(ch, f) else np.zeros(1, np.uint64)
    out.update({f: int(getattr(ch, f)) for f in CHAIN_COUNTS}, alignments=alignment_dict(al))
    return out


def chain_list(c):
    """dict of arrays shaped like Mdbg.graph_chains() -> (ChainList with HOST pointers, the arrays that must outlive it)"""
    al, keep_a = alignment_list(c["alignments"])
    keep = {f: np.ascontiguousarray(c[f], dtype=t) for f, t, _ in CHAIN_FIELDS}
    keep.update({f: np.ascontiguousarray(c[f], dtype=np.uint64) for f, _ in CHAIN_OFFSETS})
    P = lambda x: x.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(x.dtype)))
    out = ChainList(alignments=al, **{f: int(c[f]) for f in CHAIN_COUNTS})
    for f in keep:
        setattr(out, f, P(keep[f]))
    return out, (keep, keep_a)


def gaf_append_chains(path, chains, unitigs, read_lengths, truncate=False):
    """appends one GAF line per chain of a graph_chains() / chain_batch() result to `path` through libmdbg_emit's writer (mdbg_gaf_append_chains,
    include/mdbg_chain.h), the one the C program uses.  chains: the result dict or a ChainList with HOST pointers; unitigs, read_lengths: as align.gaf_append"""
    from . import emit
    from .api import MdbgError, UnitigList
    L = emit.load_library()
    ch, keep_c = (chains, None) if isinstance(chains, ChainList) else chain_list(chains)
    ul, keep_u = (unitigs, None) if isinstance(unitigs, UnitigList) else emit.unitig_list(unitigs)
    lens = np.ascontiguousarray(read_lengths, dtype=np.uint64)
    if len(lens) != int(ch.alignments.n_reads):
        raise ValueError("read_lengths has %d entries for %d reads" % (len(lens), int(ch.alignments.n_reads)))
    rc = L.mdbg_gaf_append_chains(os.fsencode(path), int(bool(truncate)), C.byref(ch), C.byref(ul), lens.ctypes.data)
    del keep_c, keep_u
    if rc:
        raise MdbgError(rc, "mdbg_gaf_append_chains")
