#!/usr/bin/env python3
"""The phasing VCF of a cohort over ONE shared index: two routes from one phasing-only job that has run to the
bytes of every multi-sample line `CHROM .. INFO GT:KC a|b:KC ...`, on 8 shared index contigs x 2 000 bubbles at 30 paths (the
reference's phasing panel), a fifth of the bubbles multiallelic, a tenth of the ALT alleles of undefined sequence, one record a
bubble: S = 64 samples (--samples 64) and one (--samples 1).  One process, one warm-up, several repeats with their spread.

  (a)  what there was before: pg_job_fetch_all (haplotypes, kept flags, k-mer counts, coverage; no bins), then in C++
       (tools/phased_lines_host_route.cpp over libpangenie_host) one GenotypingResult per bubble and Graph::phasing_records per
       sample, then the join of the samples' columns behind Graph::phasing_fixed_columns — on 1 and on 16 threads;
  (b)  the device route: pg_job_record_phase, pg_job_phased_text, pg_job_phased_lines (their kernels' ms and their wall times) +
       pg_job_phased_lines_first and pg_job_fetch_phased_lines_packed.

The fixed columns are formed once, before either route starts, and their upload (pg_job_phased_line_prefix) is not in (b)'s time.
Asserts that both routes give the same bytes and offsets.  Prints a table and one JSON line.  Sets no threshold on time.

    python tools/bench_phased_lines.py --samples 64|1 [--variants V] [--repeats N] [--build-only]
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
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

HOST_ROUTE = ROOT / "tools" / "_build" / "libphased_lines_host_route.so"
CONTIGS, PATHS = 8, 30


def build_host_route() -> Path:
    build.build_host()
    src = ROOT / "tools" / "phased_lines_host_route.cpp"
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
    ap.add_argument("--build-only", action="store_true", help="build tools/_build/libphased_lines_host_route.so and leave")
    args = ap.parse_args()
    route = C.CDLL(str(build_host_route()))
    if args.build_only:
        return
    route.pl_graphs_new.restype = C.c_void_p
    route.pl_graphs_new.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    route.pl_graphs_free.argtypes = [C.c_void_p]
    route.pl_fixed_columns.restype = C.c_uint64
    route.pl_fixed_columns.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    route.pl_host_route.restype = C.c_uint64
    route.pl_host_route.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    nc, S, V = CONTIGS, args.samples, args.variants
    index = [synthetic_panel(V, PATHS, 20, seed=777 + i, multiallelic_frac=0.2) for i in range(nc)]
    pool = []
    for s in range(min(S, 16)):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    prm = hmm.make_params(1.26, False, 1e-5, run_genotyping=False, run_phasing=True)
    job = hmm.Job.cohort(index, [pool[s % len(pool)] for s in range(S)], hmm.ProbabilityTable(*default_table_args()), prm)
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
    graphs = route.pl_graphs_new(nc, Vs.ctypes.data, PATHS, ptrs(aoffs), ptrs(undefs), ptrs(pas))
    assert graphs, "the graphs of the host route could not be made"
    for _ in range(2):
        job.run()
    lib, err = job._lib, C.create_string_buffer(1024)

    def check(rc):
        if rc:
            raise RuntimeError(err.value.decode(errors="replace"))

    # what pg_job_fetch_all fills for route (a): no bins
    n_chains = S * nc
    bufs = {k: [np.zeros(V, dt) for _ in range(n_chains)] for k, dt in (("hap1", np.uint16), ("hap2", np.uint16), ("kept", np.uint8), ("uk", np.uint16), ("kc", np.uint16))}
    results = (_lib.PgContigResult * n_chains)()
    for c in range(n_chains):
        results[c].haplotype_1 = bufs["hap1"][c].ctypes.data_as(_lib.u16p)
        results[c].haplotype_2 = bufs["hap2"][c].ctypes.data_as(_lib.u16p)
        results[c].kept = bufs["kept"][c].ctypes.data_as(_lib.u8p)
        results[c].n_kmers = bufs["uk"][c].ctypes.data_as(_lib.u16p)
        results[c].coverage = bufs["kc"][c].ctypes.data_as(_lib.u16p)
    check(lib.pg_job_fetch_all(job.h, results, err, 1024))
    # the fixed columns, once for both routes (UK as pg_job_fetch reports it: the same for every sample over a shared index)
    prefix_bytes = 0
    for k in range(nc):
        assert all(np.array_equal(bufs["uk"][s * nc + k], bufs["uk"][k]) for s in range(S))
        n = int(route.pl_fixed_columns(graphs, k, bufs["uk"][k].ctypes.data, None, None))
        off, data = np.zeros(V + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
        route.pl_fixed_columns(graphs, k, bufs["uk"][k].ctypes.data, off.ctypes.data, data.ctypes.data)
        job.record_plan(k, plans[k])
        job.phased_line_prefix(k, off, data[:n])
        prefix_bytes += n
    n_lines = nc * V
    cap = calls.record_lines_bound(n_lines, S, prefix_bytes, calls.phase_text_bound(n_lines * S))
    host_off, host_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    dev_off, dev_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    line_first, byte_first = np.zeros(nc + 1, np.uint64), np.zeros(nc + 1, np.uint64)
    seconds = np.zeros(2, np.float64)
    arg = {k: ptrs(v) for k, v in bufs.items()}

    T = {k: [] for k in ("a_fetch", "a_records_1", "a_join_1", "a_records_16", "a_join_16", "b_phase", "b_text", "b_lines", "b_fetch")}
    K = {k: [] for k in ("phase", "text", "lines")}
    n_host = n_dev = 0
    for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
        t0 = time.perf_counter()
        check(lib.pg_job_fetch_all(job.h, results, err, 1024))
        t1 = time.perf_counter()
        host = []
        for threads in (1, 16):
            n_host = route.pl_host_route(graphs, nc, S, arg["hap1"], arg["hap2"], arg["kept"], arg["uk"], arg["kc"], 0, threads, host_off.ctypes.data,
                                         host_out.ctypes.data, seconds.ctypes.data)
            host += [float(seconds[0]), float(seconds[1])]
        t2 = time.perf_counter()
        check(lib.pg_job_record_phase(job.h, err, 1024))
        t3 = time.perf_counter()
        check(lib.pg_job_phased_text(job.h, 0, err, 1024))
        t4 = time.perf_counter()
        check(lib.pg_job_phased_lines(job.h, err, 1024))
        t5 = time.perf_counter()
        check(lib.pg_job_phased_lines_first(job.h, None, line_first.ctypes.data, byte_first.ctypes.data, err, 1024))
        n_dev = int(byte_first[-1])
        check(lib.pg_job_fetch_phased_lines_packed(job.h, dev_off.ctypes.data, dev_out.ctypes.data, n_dev, err, 1024))
        t6 = time.perf_counter()
        if rep:
            for k, v in zip(T, (t1 - t0, *host, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                T[k].append(v)
            K["phase"].append(job.record_phase_ms())
            K["text"].append(job.phased_text_ms())
            K["lines"].append(job.phased_lines_ms())
    assert n_dev == n_host and np.array_equal(dev_out[:n_dev], host_out[:n_host]), (n_dev, n_host)   # both routes: the same bytes
    assert np.array_equal(dev_off, host_off) and int(line_first[-1]) == n_lines
    dots = int(np.count_nonzero(dev_out[:n_dev] == ord(".")))
    job.close()
    route.pl_graphs_free(graphs)
    ms = lambda xs, scale=1e3: (scale * float(np.median(xs)), scale * min(xs), scale * max(xs))
    fmt = lambda t: "%.3f [%.3f … %.3f]" % t
    med = lambda k: 1e3 * float(np.median(T[k]))
    rows = [("(a) `pg_job_fetch_all` (no bins)", ms(T["a_fetch"])),
            ("(a) `Graph::phasing_records` per sample, 1 thread", ms(T["a_records_1"])), ("(a) … on 16 threads", ms(T["a_records_16"])),
            ("(a) the join on the host, 1 thread", ms(T["a_join_1"])), ("(a) … on 16 threads", ms(T["a_join_16"])),
            ("(b) `pg_job_record_phase`, wall", ms(T["b_phase"])), ("(b) … its kernel (`_ms`)", ms(K["phase"], 1.0)),
            ("(b) `pg_job_phased_text`, wall", ms(T["b_text"])), ("(b) … its kernels (`_ms`)", ms(K["text"], 1.0)),
            ("(b) `pg_job_phased_lines`, wall", ms(T["b_lines"])), ("(b) … its kernels (`_ms`)", ms(K["lines"], 1.0)),
            ("(b) `_first` + packed fetch", ms(T["b_fetch"]))]
    a1 = med("a_fetch") + med("a_records_1") + med("a_join_1")
    a16 = med("a_fetch") + med("a_records_16") + med("a_join_16")
    b = med("b_phase") + med("b_text") + med("b_lines") + med("b_fetch")
    print("| ms | S = %d (%d lines, %.2f MB) |\n|---|---|" % (S, n_lines, n_dev / 1e6))
    for name, t in rows:
        print("| %s | %s |" % (name, fmt(t)))
    print("| route (a) in all: 1 thread / 16 threads | %.3f / %.3f |\n| route (b) in all | %.3f |" % (a1, a16, b))
    res = {"samples": S, "contigs": nc, "variants": V, "paths": PATHS, "lines": n_lines, "line_bytes": n_dev, "prefix_bytes": prefix_bytes, "dots_in_the_lines": dots,
           "repeats": args.repeats, "routes_agree": True, "route_a_ms": {"with_1_thread": round(a1, 3), "with_16_threads": round(a16, 3)}, "route_b_ms": round(b, 3)}
    res.update({k: {"median_ms": round(1e3 * float(np.median(v)), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)} for k, v in T.items()})
    res.update({"kernels_" + k + "_ms": {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in K.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
