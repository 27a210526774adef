#!/usr/bin/env python3
"""The sampled-panel VCF of a sampled cohort: two routes from one sampled cohort job (pg_sampler_cohort_new, 15
passes and the reference path out of 40 paths) to the bytes of every sample's lines `CHROM .. INFO GT h0 h1 ... h15`, on 8
chromosomes x 2 000 bubbles, a fifth of the bubbles multiallelic, a tenth of the ALT alleles of undefined sequence, one record a
bubble: S = 64 samples (--samples 64) and one (--samples 1).  One process, one warm-up, several repeats with their spread.

  (a)  what there was before: pg_job_fetch_panel per chain (kmer_off and path_allele of the reduced panel), then in C++
       (tools/panel_lines_host_route.cpp over libpangenie_host) one SampledPanel per bubble and Graph::sampled_panel_records per
       chain, the lines packed — on 1 and on 16 threads;
  (b)  the device route: pg_job_panel_text, pg_job_panel_lines (their kernels' ms and their wall times) +
       pg_job_panel_lines_first and pg_job_fetch_panel_lines_packed.
Route (b) starts behind route (a)'s host work, that is on a device that has idled for as long as that took; the text is therefore
formed a second time at once and that wall time printed beside (b), not as part of it.

The job, its strided plans and its slotted prefixes are ready before either route starts.  Asserts that both routes give the same
bytes and offsets.  Prints a table and one JSON line.  Sets no threshold on time.

    python tools/bench_panel_lines.py --samples 64|1 [--variants V] [--repeats N] [--build-only]
"""
import argparse
import ctypes as C
import json
import shutil
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pangenie_amd import _lib, build, calls, hmm  # noqa: E402
from pangenie_amd import sampler as smp  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

HOST_ROUTE = ROOT / "tools" / "_build" / "libpanel_lines_host_route.so"
CONTIGS, PATHS, SIZE = 8, 40, 15


def build_host_route() -> Path:
    build.build_host()
    src = ROOT / "tools" / "panel_lines_host_route.cpp"
    if not HOST_ROUTE.exists() or HOST_ROUTE.stat().st_mtime < max(src.stat().st_mtime, build.HOST_LIB.stat().st_mtime):
        HOST_ROUTE.parent.mkdir(parents=True, exist_ok=True)
        host, csrc = ROOT / "pangenie_amd" / "host", ROOT / "pangenie_amd" / "csrc"
        cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", str(src), "-o", str(HOST_ROUTE), f"-L{host}", "-lpangenie_host",
               f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", "-Wl,-rpath,$ORIGIN/../../pangenie_amd/host:$ORIGIN/../../pangenie_amd/csrc"]
        subprocess.run(cmd, check=True)
    return HOST_ROUTE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--variants", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--build-only", action="store_true", help="build tools/_build/libpanel_lines_host_route.so and leave")
    args = ap.parse_args()
    route = C.CDLL(str(build_host_route()))
    if args.build_only:
        return
    route.pp_graphs_new.restype = C.c_void_p
    route.pp_graphs_new.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    route.pp_graphs_free.argtypes = [C.c_void_p]
    route.pp_fixed_columns_slotted.restype = C.c_uint64
    route.pp_fixed_columns_slotted.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    route.pp_host_route.restype = C.c_uint64
    route.pp_host_route.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    nc, S, V, P = CONTIGS, args.samples, args.variants, SIZE + 1
    index = [synthetic_panel(V, PATHS, 20, seed=777 + i, multiallelic_frac=0.2) for i in range(nc)]
    pool = []
    for s in range(min(S, 16)):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    job, _, _ = smp.sample_cohort(index, [pool[s % len(pool)] for s in range(S)], SIZE, hmm.ProbabilityTable(*default_table_args()),
                                  hmm.make_params(1.26, False, 1e-5), add_reference=True, want_paths=False)
    n_chains = S * nc
    assert job.n_chains == n_chains
    # one record a bubble over all its allele ids, a tenth of the ALT alleles undefined: the plan of the graphs the host route prints
    rng = np.random.default_rng(20261021)
    plans, aoffs, undefs = [], [], []
    for ix in index:
        a0, aid = ix.allele_off.astype(np.int64), np.asarray(ix.allele_id)
        n_ids = [int(aid[a0[v]:a0[v + 1]].max()) + 1 for v in range(V)]
        undef = [[False] + [bool(x) for x in rng.random(n - 1) < 0.1] for n in n_ids]
        plans.append(calls.RecordPlan.from_records([[(list(range(n)), [not u for u in un])] for n, un in zip(n_ids, undef)]))
        aoffs.append(np.concatenate([[0], np.cumsum(n_ids)]).astype(np.uint32))
        undefs.append(np.array([u for un in undef for u in un], np.uint8))
    ptrs = lambda arrays: (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    Vs = np.full(nc, V, np.uint32)
    pas = [np.ascontiguousarray(ix.path_allele, np.uint16) for ix in index]
    graphs = route.pp_graphs_new(nc, Vs.ctypes.data, PATHS, ptrs(aoffs), ptrs(undefs), ptrs(pas))
    assert graphs, "the graphs of the host route could not be made"
    lib, err = job._lib, C.create_string_buffer(1024)

    def check(rc):
        if rc:
            raise RuntimeError(err.value.decode(errors="replace"))

    # the strided plans and the slotted fixed columns, once for both routes
    prefix_bytes = 0
    for k in range(nc):
        n = int(route.pp_fixed_columns_slotted(graphs, k, None, None, None))
        off, data, slot = np.zeros(V + 1, np.uint64), np.zeros(max(n, 1), np.uint8), np.zeros(V, np.uint32)
        route.pp_fixed_columns_slotted(graphs, k, off.ctypes.data, data.ctypes.data, slot.ctypes.data)
        job.record_plan_strided(k, nc, plans[k])
        job.panel_line_prefix_strided(k, nc, off, data[:n], slot=slot)
        prefix_bytes += n
    n_lines = n_chains * V
    cap = S * prefix_bytes + calls.panel_text_bound(n_lines, P) + 7 * n_lines   # (a tab, a newline and at most five digits of UK a line)
    host_off, host_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    dev_off, dev_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    line_first, byte_first = np.zeros(n_chains + 1, np.uint64), np.zeros(n_chains + 1, np.uint64)
    seconds = np.zeros(2, np.float64)
    koffs = [np.zeros(V + 1, np.uint32) for _ in range(n_chains)]
    pals = [np.zeros(V * P, np.uint16) for _ in range(n_chains)]
    koff_p, pal_p = [a.ctypes.data_as(_lib.u32p) for a in koffs], [a.ctypes.data_as(_lib.u16p) for a in pals]
    arg_koff, arg_pal = ptrs(koffs), ptrs(pals)

    T = {k: [] for k in ("a_fetch", "a_records_1", "a_pack_1", "a_records_16", "a_pack_16", "b_text", "b_lines", "b_fetch", "text_again")}
    K = {k: [] for k in ("text", "lines")}
    n_host = n_dev = 0
    for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
        t0 = time.perf_counter()
        for c in range(n_chains):
            check(lib.pg_job_fetch_panel(job.h, c, koff_p[c], None, None, None, None, None, None, pal_p[c], err, 1024))
        t1 = time.perf_counter()
        host = []
        for threads in (1, 16):
            n_host = route.pp_host_route(graphs, nc, S, P, arg_koff, arg_pal, threads, host_off.ctypes.data, host_out.ctypes.data, seconds.ctypes.data)
            host += [float(seconds[0]), float(seconds[1])]
        t2 = time.perf_counter()
        check(lib.pg_job_panel_text(job.h, err, 1024))
        t3 = time.perf_counter()
        first_kernels = job.panel_text_ms()
        check(lib.pg_job_panel_text(job.h, err, 1024))   # once more, not part of route (b): the device has just worked, not idled behind route (a)
        t3b = time.perf_counter()
        t3c = time.perf_counter()
        check(lib.pg_job_panel_lines(job.h, err, 1024))
        t4 = time.perf_counter()
        check(lib.pg_job_panel_lines_first(job.h, None, line_first.ctypes.data, byte_first.ctypes.data, err, 1024))
        n_dev = int(byte_first[-1])
        check(lib.pg_job_fetch_panel_lines_packed(job.h, dev_off.ctypes.data, dev_out.ctypes.data, n_dev, err, 1024))
        t5 = time.perf_counter()
        if rep:
            for k, v in zip(T, (t1 - t0, *host, t3 - t2, t4 - t3c, t5 - t4, t3b - t3)):
                T[k].append(v)
            K["text"].append(first_kernels)
            K["lines"].append(job.panel_lines_ms())
    assert n_dev == n_host and np.array_equal(dev_out[:n_dev], host_out[:n_host]), (n_dev, n_host)   # both routes: the same bytes
    assert np.array_equal(dev_off, host_off) and int(line_first[-1]) == n_lines
    dots = int(np.count_nonzero(dev_out[:n_dev] == ord(".")))
    job.close()
    route.pp_graphs_free(graphs)
    ms = lambda xs, scale=1e3: (scale * float(np.median(xs)), scale * min(xs), scale * max(xs))
    fmt = lambda t: "%.3f [%.3f … %.3f]" % t
    med = lambda k: 1e3 * float(np.median(T[k]))
    rows = [("(a) `pg_job_fetch_panel` per chain (kmer_off, path_allele)", ms(T["a_fetch"])),
            ("(a) `Graph::sampled_panel_records` per chain, 1 thread", ms(T["a_records_1"])), ("(a) … on 16 threads", ms(T["a_records_16"])),
            ("(a) the lines packed on the host, 1 thread", ms(T["a_pack_1"])), ("(a) … on 16 threads", ms(T["a_pack_16"])),
            ("(b) `pg_job_panel_text`, wall", ms(T["b_text"])), ("(b) … its kernels (`_ms`)", ms(K["text"], 1.0)),
            ("(b) `pg_job_panel_lines`, wall", ms(T["b_lines"])), ("(b) … its kernels (`_ms`)", ms(K["lines"], 1.0)),
            ("(b) `_first` + packed fetch", ms(T["b_fetch"])),
            ("(`pg_job_panel_text` once more at once, wall: not in (b))", ms(T["text_again"]))]
    a1 = med("a_fetch") + med("a_records_1") + med("a_pack_1")
    a16 = med("a_fetch") + med("a_records_16") + med("a_pack_16")
    b = med("b_text") + med("b_lines") + med("b_fetch")
    print("| ms | S = %d (%d lines, %.2f MB) |\n|---|---|" % (S, n_lines, n_dev / 1e6))
    for name, t in rows:
        print("| %s | %s |" % (name, fmt(t)))
    print("| route (a) in all: 1 thread / 16 threads | %.3f / %.3f |\n| route (b) in all | %.3f |" % (a1, a16, b))
    res = {"samples": S, "contigs": nc, "variants": V, "paths": P, "lines": n_lines, "line_bytes": n_dev, "prefix_bytes": prefix_bytes, "dots_in_the_lines": dots,
           "repeats": args.repeats, "routes_agree": True, "route_a_ms": {"with_1_thread": round(a1, 3), "with_16_threads": round(a16, 3)}, "route_b_ms": round(b, 3)}
    res.update({k: {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)} for k, v in T.items()})
    res.update({"kernels_" + k + "_ms": {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in K.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
