"""bench.py's launcher contract and the RCCL id hand-over, as far as they can be checked without a GPU."""
import ctypes as C
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_gpus_n_without_n_gpus_fails_loudly():
    """`python bench.py --gpus 2` must never print an N=1 line: with fewer than 2 visible GPUs it exits non-zero and says why"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2 needs 2 GPUs" in r.stderr and r.stdout.strip() == ""


def test_bench_world_size_must_match_gpus_flag():
    """a launcher that starts 2 ranks while the command line says --gpus 1 (or the reverse) is a configuration error, not a mislabelled line"""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "--gpus 1 but the launcher started 2 rank(s)" in r.stderr and r.stdout.strip() == ""


def test_bench_human_workload_needs_a_divisor_of_its_shards():
    """--workload human is the same eight shards at every N: a rank count that does not divide them is refused before anything runs"""
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "--gpus must divide 8" in r.stderr and r.stdout.strip() == ""


def test_nccl_unique_id_travels_whole():
    """the 128-byte ncclUniqueId is binary: a NUL byte inside must not shorten what rank 0 broadcasts (rust_mdbg_amd/dist_c.py)"""
    from rust_mdbg_amd.dist_c import UniqueId
    uid = UniqueId()
    raw = bytes([7, 9, 0, 3] + [0] * 60 + list(range(1, 65)))
    C.memmove(C.byref(uid), raw, 128)
    assert bytes(uid.internal) != raw                      # the trap: c_char arrays convert like C strings
    blob = C.string_at(C.byref(uid), C.sizeof(uid))         # what rccl_comm() sends
    assert blob == raw and len(blob) == 128
    back = UniqueId()
    C.memmove(C.byref(back), blob, C.sizeof(back))
    assert C.string_at(C.byref(back), 128) == raw


def test_bench_steps_must_be_positive():
    """--steps sets the number of timed steps: none at all is refused before anything runs"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


def _host_table(n, k, seed):
    """a node table in host memory shaped like mdbg_nodes (rows in a shuffled order, as a hash table leaves them)"""
    import numpy as np
    from rust_mdbg_amd import api
    rng = np.random.default_rng(seed)
    cols = {"keys": rng.integers(0, 1 << 64, size=(n, k), dtype=np.uint64, endpoint=False), "index": rng.permutation(3 * n)[:n].astype(np.uint32),
            "abundance": rng.integers(2, 1 << 16, n).astype(np.uint16), "seqlen": rng.integers(0, 1 << 32, n).astype(np.uint32),
            "shift": rng.integers(0, 1 << 16, (n, 2)).astype(np.uint16), "shift_full": rng.integers(0, 1 << 40, (n, 2)).astype(np.uint64),
            "src_read": rng.integers(0, 1 << 52, n).astype(np.uint64), "src_start": rng.integers(0, 1 << 20, n).astype(np.uint64),
            "src_end": rng.integers(0, 1 << 20, n).astype(np.uint64), "reversed": rng.integers(0, 2, n).astype(np.uint8)}
    nd = api.Nodes(n=n, k=k, n_distinct=2 * n, n_wrapped=0)
    for f, a in cols.items():
        setattr(nd, f, a.ctypes.data_as(dict(api.Nodes._fields_)[f]))
    return nd, cols


def _host_copy(ptr, nbytes, dtype):
    import numpy as np
    return np.frombuffer(C.string_at(ptr, nbytes), dtype=dtype).copy()


def _load_dump(d):
    import numpy as np
    out = {}
    for f in sorted(os.listdir(d)):
        a = np.load(os.path.join(d, f))
        assert f.endswith(".npy") and a.dtype == np.float64, f
        out[f[:-4]] = a
    return out


def test_dump_outputs_writes_the_table_in_index_order(tmp_path, monkeypatch):
    """bench.py --dump-outputs on a host-memory table: every row when the table fits, in DbgEntry.index order, keys exact through their 32-bit halves,
    and the gather is the same when the copies go chunk by chunk"""
    import numpy as np
    import bench
    nd, cols = _host_table(500, 7, seed=1)
    bench.dump_outputs(str(tmp_path / "a"), nd, _host_copy, lambda: (0xFEDCBA9876543210, 0x0123456789ABCDEF), [500, 500, 1000, 0])
    monkeypatch.setattr(bench, "DUMP_CHUNK_BYTES", 100)
    bench.dump_outputs(str(tmp_path / "b"), nd, _host_copy, lambda: (0xFEDCBA9876543210, 0x0123456789ABCDEF), [500, 500, 1000, 0])
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    assert set(a) == set(b) and all(np.array_equal(a[f], b[f]) for f in a)
    order = np.argsort(cols["index"])
    keys = (a["keys_hi32"].astype(np.uint64) << np.uint64(32)) | a["keys_lo32"].astype(np.uint64)
    assert np.array_equal(keys, cols["keys"][order])
    for f in ("index", "abundance", "seqlen", "shift", "shift_full", "src_read", "src_start", "src_end", "reversed"):
        assert np.array_equal(a[f], cols[f][order].astype(np.float64)), f
    assert a["node_digest"].tolist() == [0xFEDCBA98, 0x76543210, 0x01234567, 0x89ABCDEF] and a["node_counts"].tolist() == [500, 500, 1000, 0]


def test_dump_outputs_samples_a_large_table_within_its_budget(tmp_path):
    """a table over the budget: a fixed seeded sample of its rows (the same in every run), still in index order, and the files stay under the 64 MB bench.py promises"""
    import numpy as np
    import bench
    nd, cols = _host_table(120000, 35, seed=2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), nd, _host_copy, lambda: (1, 2), [120000, 120000, 240000, 0])
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    assert all(np.array_equal(a[f], b[f]) for f in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    n_s = len(a["index"])
    assert 50000 < n_s < 120000 and a["keys_hi32"].shape == (n_s, 35) and np.all(np.diff(a["index"]) > 0)
    pos = {int(v): i for i, v in enumerate(cols["index"])}
    rows = np.array([pos[int(v)] for v in a["index"]])
    keys = (a["keys_hi32"].astype(np.uint64) << np.uint64(32)) | a["keys_lo32"].astype(np.uint64)
    assert np.array_equal(keys, cols["keys"][rows]) and np.array_equal(a["src_read"], cols["src_read"][rows].astype(np.float64))
