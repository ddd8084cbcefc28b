"""CPU-side checks of the drop-in boundary: the library loads and exports every symbol include/mdbg_hip.h declares, every ctypes mirror
has the layout gcc gives the headers' structs, and every prototype the binding declares is the header's (no compute calls — there is no GPU here)."""
import os
import re

from conftest import ROOT


def declared_symbols():
    h = open(os.path.join(ROOT, "include", "mdbg_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(mdbg_[a-z_0-9]+)\s*\(", h)))


def test_library_exports_every_declared_symbol():
    from rust_mdbg_amd import api
    L = api.load_library()
    syms = declared_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(api.EXPORTS) == syms
    assert L.mdbg_abi_version() == 3
    assert L.mdbg_strerror(0) == b"ok" and b"ACGTN" in L.mdbg_strerror(-2)


def test_build_hook_checks_agree_with_the_tree():
    """the checks __graft_entry__.build() runs behind the compile step (it once kept an ABI version of its own)"""
    import __graft_entry__ as G
    G.check_built()


def test_emit_library_exports_every_declared_symbol():
    from rust_mdbg_amd import emit
    h = open(os.path.join(ROOT, "include", "mdbg_emit.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    syms = sorted(set(re.findall(r"\b(mdbg_(?:emit|seqfile|reader|pack|packed|lmer)_[a-z_0-9]+)\s*\(", h)))
    L = emit.load_library()
    assert syms == sorted(emit.EXPORTS + emit.READER_EXPORTS)
    for s in syms:
        assert hasattr(L, s), s


# ---- every mirror against gcc's layout, every declared prototype against its header -----------------------------------------------------------------------------------
def mirrors():
    """C type name -> the ctypes class that mirrors it: written once, here"""
    from rust_mdbg_amd import api, dist_c, emit
    return {"mdbg_params": api.Params, "mdbg_nodes": api.Nodes, "mdbg_stats": api.Stats, "mdbg_packed_batch": api.PackedBatch, "mdbg_routed_lists": api.RoutedLists,
            "mdbg_edge_list": api.EdgeList, "mdbg_unitig_list": api.UnitigList, "mdbg_simplify_step": api.SimplifyStep, "mdbg_simplify_stats": api.SimplifyStats,
            "mdbg_component_list": api.ComponentList, "mdbg_contig_seqs": api.ContigSeqs, "mdbg_node_seqs": api.NodeSeqs, "mdbg_read_path_list": api.ReadPathList,
            "mdbg_junction_list": api.JunctionList, "mdbg_transit_list": api.TransitList, "mdbg_sketch_store": api.SketchStore, "mdbg_batch_info": api.BatchInfo,
            "mdbg_synth_params": api.SynthParams, "mdbg_xfer": dist_c.Xfer, "mdbg_comm": dist_c.Comm, "mdbg_edges": emit.Edges}


def layout_errors(tmp_path, by_name):
    """compiles ONE C file that prints sizeof of every struct of by_name and offsetof / sizeof of every field its mirror declares, as gcc lays out the headers' own
    definitions -> ["<struct>[.<field>]: ..."] for every figure where ctypes disagrees"""
    import ctypes as C
    import subprocess
    lines = []
    for t, cls in by_name.items():
        lines.append('printf("%s %%zu 0\\n", sizeof(%s));' % (t, t))
        lines += ['printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (t, f[0], t, f[0], t, f[0]) for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdbg_dist.h"\n#include "mdbg_emit.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = {w[0]: (int(w[1]), int(w[2])) for w in (ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    want = {}
    for t, cls in by_name.items():
        want[t] = (C.sizeof(cls), 0)
        want.update({"%s.%s" % (t, f[0]): (getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_})
    assert set(got) == set(want)
    return ["%s: gcc %s, ctypes %s" % (key, got[key], want[key]) for key in want if got[key] != want[key]]


def test_every_mirror_has_the_layout_gcc_gives_the_headers(tmp_path):
    """size of every mirrored struct, offset and size of every field (`reserved` members included; the names come from the classes' _fields_, so a new field cannot be
    forgotten), and no ctypes.Structure of the binding outside the map; then the check itself on a mirror with two fields of different size swapped"""
    import ctypes as C
    from rust_mdbg_amd import api, dist_c, emit
    by_name = mirrors()
    classes = {v for m in (api, dist_c, emit) for v in vars(m).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    # (ncclUniqueId is RCCL's, not a struct of include/: tests/test_bench_cli_cpu.py holds its 128 bytes)
    assert classes - {dist_c.UniqueId} == set(by_name.values()) and len(set(by_name.values())) == 18 + 2 and emit.Edges is api.EdgeList
    assert all(cls._fields_[-1][0] == "reserved" for cls in (api.Params, api.Stats, api.UnitigList, api.SynthParams))
    assert layout_errors(tmp_path, by_name) == []

    class Swapped(C.Structure):          # mdbg_nodes with n (8 bytes) and k (4 bytes) in each other's place
        _fields_ = [api.Nodes._fields_[1], api.Nodes._fields_[0]] + api.Nodes._fields_[2:]
    bad = layout_errors(tmp_path, dict(by_name, mdbg_nodes=Swapped))
    assert bad and all(e.startswith("mdbg_nodes.") for e in bad) and {e.split(":")[0] for e in bad} >= {"mdbg_nodes.n", "mdbg_nodes.k"}, bad


PROTOTYPE = re.compile(r"^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*\b(mdbg_\w+)[ \t]*\(([^;{}]*)\)[ \t]*;", re.M)
C_KINDS = {"void": "void", "int": "i32", "int32_t": "i32", "uint32_t": "i32", "unsigned": "i32", "uint64_t": "i64", "int64_t": "i64", "size_t": "i64", "float": "float",
           "double": "double"}


def c_kind(decl):
    """a C parameter or return type -> (kind, pointee type name or None); kinds: pointer, i32, i64, float, double, void"""
    words = re.findall(r"\w+", decl.replace("const", " "))
    if "*" in decl or "(" in decl:
        return "pointer", words[0]
    return C_KINDS[words[0]], None


def ctypes_kind(t):
    """the same of a restype / argtypes entry; the pointee only where it is a ctypes.Structure"""
    import ctypes as C
    if t is None:
        return "void", None
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "pointer", t._type_ if issubclass(t._type_, C.Structure) else None
    if t in (C.c_void_p, C.c_char_p):
        return "pointer", None
    if issubclass(t, C.Structure):
        return "struct", t
    return {C.c_float: "float", C.c_double: "double"}.get(t, "i%d" % (8 * C.sizeof(t))), None


def split_params(args):
    out, depth, cur = [], 0, ""
    for ch in args:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    out = [p.strip() for p in out + [cur]]
    return [] if out in ([""], ["void"]) else out


def prototype_errors(header_text, table, by_name):
    """every prototype `ret name(args);` of a header against its row `name -> (restype, argtypes)` -> ["<name>: ..."]: the two sets of names, the number of parameters,
    the kind of every parameter and of the return, and where the row names a mirrored struct behind a pointer, that the header names the same one.  argtypes None
    (nothing declared) passes only for a function without parameters"""
    found = {name: (ret, split_params(args)) for ret, name, args in PROTOTYPE.findall(re.sub(r"/\*.*?\*/", "", header_text, flags=re.S))}
    errs = ["%s: in the header, not in the table" % n for n in found if n not in table] + ["%s: in the table, not in the header" % n for n in table if n not in found]
    for name in (n for n in found if n in table):
        (ret, params), (restype, argtypes) = found[name], table[name]
        if argtypes is None and params:
            errs.append("%s: %d parameters in the header, no argtypes declared" % (name, len(params)))
            continue
        argtypes = tuple(argtypes or ())
        if len(params) != len(argtypes):
            errs.append("%s: %d parameters in the header, %d in the table" % (name, len(params), len(argtypes)))
            continue
        for what, c, t in [("return", ret, restype)] + [("parameter %d" % (i + 1), c, t) for i, (c, t) in enumerate(zip(params, argtypes))]:
            (ck, cp), (tk, tp) = c_kind(c), ctypes_kind(t)
            if ck != tk:
                errs.append("%s: %s is `%s` (%s), the table says %s" % (name, what, " ".join(c.split()), ck, tk))
            elif tp is not None and by_name.get(cp) is not tp:          # (a pointer the table types as c_void_p passes as a pointer)
                errs.append("%s: %s points to %s, the table to %s" % (name, what, cp, tp.__name__))
    return errs


def declared(L, header_text):
    """what the binding has declared on the loaded library L for every prototype of a header: name -> (restype, argtypes) as ctypes holds them (c_int and None where
    nothing was said)"""
    names = [name for _, name, _ in PROTOTYPE.findall(re.sub(r"/\*.*?\*/", "", header_text, flags=re.S))]
    return {n: (getattr(L, n).restype, getattr(L, n).argtypes) for n in names}


# The gaps the check finds in the binding as it stands, listed so that a new one fails:
# called without a declaration: nothing checks its arguments, and a uint64_t among them would be cut to 32 bits (tests/test_gpu_round6.py declares it for itself)
UNDECLARED = ["mdbg_dbg_segments_ms"]
# `void` in the header, restype left at ctypes' c_int: the call hands back whatever the register holds; no caller reads it
VOID_AS_INT = {"mdbg_emit.h": ["mdbg_emit_destroy: return is `void` (void), the table says i32"],
               "mdbg_dist.h": ["mdbg_dist_destroy: return is `void` (void), the table says i32"]}


def test_every_declared_prototype_agrees_with_its_header(tmp_path):
    """what rust_mdbg_amd declares on the two libraries (api.load_library; emit.load_library and a Reader; a DistMdbg for include/mdbg_dist.h) against the prototypes of
    the three headers; then the check itself on broken copies of the rows: each broken row is reported, by name, and nothing else"""
    import ctypes as C
    from rust_mdbg_amd import api, dist_c, emit
    by_name = mirrors()
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("mdbg_hip.h", "mdbg_dist.h", "mdbg_emit.h")}
    assert PROTOTYPE.findall("int (*exchange)(void* self);\ntypedef struct mdbg_dist mdbg_dist;\n") == []          # members and typedefs are no prototypes
    # include/mdbg_hip.h: declared when the library is loaded
    good = declared(api.load_library(), text["mdbg_hip.h"])
    assert len(good) == 82 and sorted(good) == sorted(api.EXPORTS)
    errs = prototype_errors(text["mdbg_hip.h"], good, by_name)
    # (a subset: in a process where tests/test_gpu_round6.py has run before, the one gap is closed)
    assert {e.split(":")[0] for e in errs} <= set(UNDECLARED) and all("no argtypes declared" in e for e in errs), errs
    # include/mdbg_emit.h: the emitter's when the library is loaded, the reader's by a Reader and its packed batches
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n")
    with emit.Reader(str(fa), device_buffers=True) as r:
        assert len(list(r.batches_packed())) == 1
    rows = declared(emit.load_library(), text["mdbg_emit.h"])
    assert len(rows) == 29 and sorted(rows) == sorted(emit.EXPORTS + emit.READER_EXPORTS)
    assert prototype_errors(text["mdbg_emit.h"], rows, by_name) == VOID_AS_INT["mdbg_emit.h"]
    # include/mdbg_dist.h: declared by every DistMdbg before it creates anything (k = 1 is refused as a parameter, with or without a device)
    try:
        dist_c.DistMdbg(1, 12, 0.01, 2, 0, 1, transport="host")
        raise AssertionError("k = 1 was accepted")
    except api.MdbgError as e:
        assert e.code == api.MDBG_E_PARAM
    rows = declared(api.load_library(), text["mdbg_dist.h"])
    assert len(rows) == 13 and prototype_errors(text["mdbg_dist.h"], rows, by_name) == VOID_AS_INT["mdbg_dist.h"]
    # the check on broken rows
    vp, u32, u64, i32, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER
    good = {n: r for n, r in good.items() if n not in UNDECLARED}
    only = lambda table: [e for e in prototype_errors(text["mdbg_hip.h"], table, by_name) if e.split(":")[0] not in UNDECLARED]
    assert only(good) == [] and tuple(good["mdbg_rewind"][1]) == (vp, u64) and tuple(good["mdbg_insert_records"][1]) == (vp, vp, u64) and good["mdbg_create"][0] is vp
    broken = {"mdbg_ingest_batch": (i32, good["mdbg_ingest_batch"][1][:-1]),          # one parameter dropped
              "mdbg_rewind": (i32, (vp, u32)),                                          # u32 where the header has uint64_t
              "mdbg_insert_records": (i32, (vp, u64, u64)),                             # an integer where the header has a pointer
              "mdbg_create": (i32, good["mdbg_create"][1]),                             # the restype left at ctypes' default for a pointer return
              "mdbg_get_stats": (i32, (vp, P(api.Nodes))),                              # a pointer to the wrong mirror
              "mdbg_sync": (i32, None)}                                                 # nothing declared for a function with parameters
    for name, row in broken.items():
        errs = only(dict(good, **{name: row}))
        assert len(errs) == 1 and errs[0].startswith(name + ": "), (name, errs)
    assert only(dict(good, mdbg_no_such_call=(i32, ()))) == ["mdbg_no_such_call: in the table, not in the header"]
    assert only({n: r for n, r in good.items() if n != "mdbg_mark"}) == ["mdbg_mark: in the header, not in the table"]


def test_create_without_gpu_fails_cleanly():
    """no silent CPU fallback: without a device mdbg_create reports MDBG_E_DEVICE"""
    import torch
    import pytest
    import rust_mdbg_amd as R
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(R.MdbgError) as e:
        R.Mdbg(5, 12, 0.01)
    assert e.value.code == -4
    with pytest.raises(R.MdbgError) as e:
        R.Mdbg(1, 12, 0.01)
    assert e.value.code == -1


def test_the_built_library_is_a_product_build():
    """mdbg_build_flags() == 0: the in-tree library is the Makefile's build (no build flag is defined);
    the host-memory calls work without a device (ordinary memory until an ingest call sees it)"""
    from rust_mdbg_amd import api
    L = api.load_library()
    assert L.mdbg_build_flags() == 0 and L.mdbg_abi_version() > 0
    p = L.mdbg_host_alloc(1 << 16)
    assert p and p % 4096 == 0 and L.mdbg_host_is_pinned(p) == 0
    L.mdbg_host_free(p)
    L.mdbg_host_free(None)


def test_headers_are_plain_c_and_the_example_links(tmp_path):
    """include/*.h must be usable from C (the drop-in boundary is a C ABI): the plain-C example host compiles with gcc -std=c99
    and links against the two libraries (running it needs a GPU: tests/test_gpu_pipeline.py)"""
    import subprocess
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    exe = str(tmp_path / "mdbg_cli")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mdbg_cli.c"), "-L" + lib, "-lmdbg_hip", "-lmdbg_emit", "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True)
    assert os.path.exists(exe)


def test_dist_header_symbols_and_c_example_link(tmp_path):
    """include/mdbg_dist.h: every declared entry point is exported, and the plain-C multi-rank example compiles as C99 and links
    (running it needs a GPU: tests/test_gpu_dist_c.py)"""
    import subprocess
    from rust_mdbg_amd import api
    h = open(os.path.join(ROOT, "include", "mdbg_dist.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    syms = sorted(set(re.findall(r"\b(mdbg_(?:dist|comm)_[a-z_0-9]+)\s*\(", h)))
    assert syms == ["mdbg_comm_rccl", "mdbg_dist_create", "mdbg_dist_ctx", "mdbg_dist_destroy", "mdbg_dist_finalize", "mdbg_dist_ingest_batch_device",
                    "mdbg_dist_ingest_batch_packed_device", "mdbg_dist_reset", "mdbg_dist_set_exchange", "mdbg_dist_set_pipeline", "mdbg_dist_stage_ms", "mdbg_dist_stage_name",
                    "mdbg_dist_traffic"]
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), s
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mdbg_dist_threads.c"), "-L" + lib, "-lmdbg_hip", "-lpthread", "-Wl,-rpath," + lib,
                    "-o", str(tmp_path / "mdbg_dist_threads")], check=True)
