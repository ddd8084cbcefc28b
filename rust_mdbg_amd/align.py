"""ctypes binding of include/mdbg_align.h — alignments of reads and query sequences on the unitig graph, and their GAF lines.

The calls on a context are methods of api.Mdbg (graph_alignments, graph_alignments_device, alignments_ms, align_batch); this module holds what they share:
the struct mirror, the column table, the prototypes (declared once, on the library api.load_library / emit.load_library has loaded) and the GAF writer."""
import ctypes as C
import os

import numpy as np


class AlignmentList(C.Structure):      # mdbg_alignment_list
    _fields_ = [("first_read", C.c_uint64), ("n_reads", C.c_uint64), ("n_windows", C.c_uint64), ("n_placed", C.c_uint64), ("n_steps", C.c_uint64),
                ("n_chained", C.c_uint64), ("n_alignments", C.c_uint64), ("n_wraps", C.c_uint64), ("n_unitigs", C.c_uint64),
                ("ordinal", C.POINTER(C.c_uint64)), ("read_windows", C.POINTER(C.c_uint32)), ("step_offsets", C.POINTER(C.c_uint64)), ("aln_offsets", C.POINTER(C.c_uint64)),
                ("first_window", C.POINTER(C.c_uint32)), ("step_windows", C.POINTER(C.c_uint32)), ("unitig", C.POINTER(C.c_uint32)), ("first_entry", C.POINTER(C.c_uint32)),
                ("strand", C.POINTER(C.c_uint8)), ("step_record", C.POINTER(C.c_uint32)), ("aln_step_offsets", C.POINTER(C.c_uint64)),
                ("aln_windows", C.POINTER(C.c_uint32)), ("query_begin", C.POINTER(C.c_uint32)), ("query_end", C.POINTER(C.c_uint32)),
                ("path_length", C.POINTER(C.c_uint64)), ("path_begin", C.POINTER(C.c_uint64)), ("path_end", C.POINTER(C.c_uint64))]


# (field, dtype, what it has one element of: "read", "step" or "alignment"); the three offset columns have one element more: ALIGNMENT_OFFSETS
ALIGNMENT_FIELDS = (("ordinal", np.uint64, "read"), ("read_windows", np.uint32, "read"), ("first_window", np.uint32, "step"), ("step_windows", np.uint32, "step"),
                    ("unitig", np.uint32, "step"), ("first_entry", np.uint32, "step"), ("strand", np.uint8, "step"), ("step_record", np.uint32, "step"),
                    ("aln_windows", np.uint32, "alignment"), ("query_begin", np.uint32, "alignment"), ("query_end", np.uint32, "alignment"),
                    ("path_length", np.uint64, "alignment"), ("path_begin", np.uint64, "alignment"), ("path_end", np.uint64, "alignment"))
ALIGNMENT_OFFSETS = (("step_offsets", "read"), ("aln_offsets", "read"), ("aln_step_offsets", "alignment"))
ALIGNMENT_COUNTS = ("n_reads", "n_windows", "n_placed", "n_steps", "n_chained", "n_alignments", "n_wraps")      # what adds up over the ranges of a partition of the reads
NO_RECORD = 0xFFFFFFFF

HIP_EXPORTS = ["mdbg_graph_alignments", "mdbg_graph_alignments_device", "mdbg_alignments_ms", "mdbg_graph_align_batch", "mdbg_graph_align_batch_device"]
EMIT_EXPORTS = ["mdbg_gaf_append"]


def declare_hip(L):
    """the prototypes of include/mdbg_align.h that libmdbg_hip exports, on the loaded library"""
    vp, u64 = C.c_void_p, C.c_uint64
    L.mdbg_graph_alignments.argtypes = [vp, u64, u64, C.POINTER(AlignmentList)]
    L.mdbg_graph_alignments_device.argtypes = [vp, u64, u64, C.POINTER(AlignmentList)]
    L.mdbg_alignments_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.mdbg_graph_align_batch.argtypes = [vp, vp, vp, u64, C.POINTER(AlignmentList)]
    L.mdbg_graph_align_batch_device.argtypes = [vp, vp, vp, u64, C.POINTER(AlignmentList)]
    for f in HIP_EXPORTS:
        getattr(L, f).restype = C.c_int


def declare_emit(L):
    """the writer of include/mdbg_align.h that libmdbg_emit exports, on the loaded library"""
    from .api import UnitigList
    L.mdbg_gaf_append.argtypes = [C.c_char_p, C.c_int, C.POINTER(AlignmentList), C.POINTER(UnitigList), C.c_void_p]
    L.mdbg_gaf_append.restype = C.c_int


def alignment_dict(al):
    """an AlignmentList with HOST pointers, copied -> dict by field name"""
    from .api import _np
    n = dict(read=int(al.n_reads), step=int(al.n_steps), alignment=int(al.n_alignments))
    out = {f: _np(getattr(al, f), n[per], t) for f, t, per in ALIGNMENT_FIELDS}
    for f, per in ALIGNMENT_OFFSETS:
        out[f] = _np(getattr(al, f), n[per] + 1, np.uint64) if getattr(al, f) else np.zeros(1, np.uint64)
    out.update({f: int(getattr(al, f)) for f in ALIGNMENT_COUNTS}, first_read=int(al.first_read), n_unitigs=int(al.n_unitigs))
    return out


def alignment_list(a):
    """dict of arrays shaped like Mdbg.graph_alignments() -> (AlignmentList with HOST pointers, the arrays that must outlive it)"""
    keep = {f: np.ascontiguousarray(a[f], dtype=t) for f, t, _ in ALIGNMENT_FIELDS}
    keep.update({f: np.ascontiguousarray(a[f], dtype=np.uint64) for f, _ in ALIGNMENT_OFFSETS})
    P = lambda x: x.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(x.dtype)))
    out = AlignmentList(first_read=int(a.get("first_read", 0)), n_unitigs=int(a.get("n_unitigs", 0)), **{f: int(a[f]) for f in ALIGNMENT_COUNTS})
    for f in keep:
        setattr(out, f, P(keep[f]))
    return out, keep


def gaf_append(path, alignments, unitigs, read_lengths, truncate=False):
    """appends the GAF lines of one graph_alignments() / align_batch() result to `path` through libmdbg_emit's writer (mdbg_gaf_append, include/mdbg_align.h), the one
    the C program uses.  alignments: the result dict or an AlignmentList with HOST pointers; unitigs: the list the alignments were made on (the dict of graph_unitigs()
    or a UnitigList with HOST pointers); read_lengths[q]: the raw length of read first_read + q"""
    from . import emit
    from .api import MdbgError, UnitigList
    L = emit.load_library()
    al, keep_a = (alignments, None) if isinstance(alignments, AlignmentList) else alignment_list(alignments)
    ul, keep_u = (unitigs, None) if isinstance(unitigs, UnitigList) else emit.unitig_list(unitigs)
    lens = np.ascontiguousarray(read_lengths, dtype=np.uint64)
    if len(lens) != int(al.n_reads):
        raise ValueError("read_lengths has %d entries for %d reads" % (len(lens), int(al.n_reads)))
    rc = L.mdbg_gaf_append(os.fsencode(path), int(bool(truncate)), C.byref(al), C.byref(ul), lens.ctypes.data)
    del keep_a, keep_u
    if rc:
        raise MdbgError(rc, "mdbg_gaf_append")
