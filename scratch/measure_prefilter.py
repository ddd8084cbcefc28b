"""The counting pre-filter (MDBG_FLAG_PREFILTER) against the exact mode of the same build, on one GPU: per store the time of the count pass, the admit pass and the
gated insertion beside the exact insertion's, finalize, table and filter bytes, admitted / all windows, promoted singletons at the default filter size.

Stores: BASELINE configs[1] (100 k reads of ~15 kb, k=21 l=12 d=0.003), configs[2] (140 Mb @50x, k=35 l=12 d=0.002), and configs[1]'s shape with err_ppm raised
until at least 80 % of the distinct keys are seen once.  One warm-up pass, then the median of 10.  How the parts are separated (the library has one insertion timer):
  exact insert  = mdbg_stats.ms_insert of the exact context (device events around the insert kernels)
  count         = host time of (sketch + count) minus host time of the sketch alone, both bracketed by mdbg_sync
  gated insert  = mdbg_stats.ms_insert of the pre-filter context (the same events, around the gated kernels)
  admit         = host time of mdbg_insert_resident minus the gated insert (it also holds the round's two host round trips and the window count)
usage: python scratch/measure_prefilter.py [store ...]      stores: c1 c2 noisy (default: all)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_mdbg_amd as R

STORES = {"c1": dict(k=21, l=12, d=0.003, genome=100_000_000, n_reads=100_000, err_ppm=1000),
          "c2": dict(k=35, l=12, d=0.002, genome=140_000_000, n_reads=int(140e6 * 50 / 15000), err_ppm=1000),
          "noisy": dict(k=21, l=12, d=0.003, genome=100_000_000, n_reads=100_000, err_ppm=None)}
REPS = 10


def make(cfg, prefilter):
    return R.Mdbg(cfg["k"], cfg["l"], cfg["d"], 2, device=0, prefilter=prefilter)


def one_pass(m, cfg, db, do, nb, prefilter):
    t = {}
    m.reset(0)
    m.sync(); t0 = time.perf_counter()
    if prefilter:
        m.ingest_device(db, do, cfg["n_reads"], nb, 0)          # sketch + count
    else:
        m.sketch_device(db, do, cfg["n_reads"], nb, 0)
    m.sync(); t["sketch(+count)"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    m.insert_resident()
    m.sync(); t["insert_resident"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    nd = m.finalize_device()
    m.sync(); t["finalize"] = (time.perf_counter() - t0) * 1e3
    st = m.stats()
    t["ms_insert"] = st["ms_insert"]; t["ms_finalize"] = st["ms_finalize"]; t["ms_sketch"] = st["ms_sketch"]
    return t, st, int(nd.n), int(nd.n_distinct)


def measure(name):
    cfg = dict(STORES[name])
    out = {"store": name, "params": {f: cfg[f] for f in ("k", "l", "d", "n_reads")}}
    src = make(cfg, False)          # owns the synthetic reads for both contexts
    errs = [cfg["err_ppm"]] if cfg["err_ppm"] else [20000, 40000, 60000, 80000, 120000]
    for err in errs:
        db, do, nb = src.synth_reads_device(seed=1, genome_len=cfg["genome"], n_reads=cfg["n_reads"], err_ppm=err)
        with make(cfg, False) as probe:          # the share of keys seen once: distinct keys at A = 2 against the nodes
            probe.ingest_device(db, do, cfg["n_reads"], nb, 0)
            nd = probe.finalize_device()
            distinct, nodes = int(nd.n_distinct), int(nd.n)
        share = 1.0 - nodes / max(1, distinct)
        if cfg["err_ppm"] or share >= 0.8:
            break
    out.update(err_ppm=err, gbases=nb / 1e9, distinct_keys=distinct, nodes=nodes, singleton_share=round(share, 4))
    res = {}
    for mode in ("exact", "prefilter"):
        with make(cfg, mode == "prefilter") as m:
            runs = []
            for rep in range(REPS + 1):
                t, st, n, nbefore = one_pass(m, cfg, db, do, nb, mode == "prefilter")
                if rep:
                    runs.append(t)
            res[mode] = dict({f: round(statistics.median(r[f] for r in runs), 3) for f in runs[0]}, nodes=n, n_distinct=nbefore, n_windows=st["n_windows"],
                             n_windows_admitted=st["n_windows_admitted"], table_capacity=st["table_capacity"], table_bytes=st["table_capacity"] * 32,
                             filter_bytes=st["prefilter_cells"] // 4)
    e, p = res["exact"], res["prefilter"]
    assert e["nodes"] == p["nodes"] == nodes
    out["exact"], out["prefilter"] = e, p
    out["derived"] = dict(count_ms=round(p["sketch(+count)"] - e["sketch(+count)"], 3), admit_ms=round(p["insert_resident"] - p["ms_insert"], 3), gated_insert_ms=p["ms_insert"],
                          exact_insert_ms=e["ms_insert"], exact_insert_call_ms=e["insert_resident"], finalize_ms=(e["ms_finalize"], p["ms_finalize"]),
                          admitted_share=round(p["n_windows_admitted"] / max(1, p["n_windows"]), 4), promoted_singletons=p["n_distinct"] - nodes,
                          table_bytes_saved=e["table_bytes"] - p["table_bytes"],
                          step_ms=(round(e["sketch(+count)"] + e["insert_resident"] + e["finalize"], 3), round(p["sketch(+count)"] + p["insert_resident"] + p["finalize"], 3)))
    src.close()
    return out


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(STORES)):
        print(json.dumps(measure(name)), flush=True)
