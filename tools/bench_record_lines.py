#!/usr/bin/env python3
"""Whole multi-sample VCF lines of a cohort over ONE shared index: two routes from one job that has run and
formed its record text to the bytes of every line, on the `small` shape of tools/bench_sampled_record_fields.py (8 contigs x
2 000 bubbles, its plan) reshaped to a shared-index cohort at 16 paths: 512 samples (--samples 512) and one (--samples 1),
prefixes of about 60 bytes.  One process, one warm-up, several repeats with their spread.

  (a)  what there was before: pg_job_fetch_record_text_packed, then the join on the host in C++
       (tools/record_lines_host_join.cpp: lengths, their sum, copies) on 1 and on 16 threads;
  (b)  the device route: pg_job_record_lines (its kernels' ms and its wall time) + pg_job_fetch_record_lines_packed.

Asserts that both routes give the same bytes and offsets.  Prints one JSON line: median [min .. max] of each part and the
kernels' achieved GB/s against their formula traffic.  Sets no threshold on time.

    python tools/bench_record_lines.py --samples 512|1 [--shape tiny|small] [--repeats N] [--build-only]
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
sys.path.insert(0, str(ROOT / "tools"))

from bench_record_calls import random_plan  # noqa: E402
from bench_sampled_record_fields import SHAPES  # noqa: E402
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

HOST_JOIN = ROOT / "tools" / "_build" / "librecord_lines_host_join.so"
PATHS = 16
HBM_PEAK_GBPS = 8000.0


def build_host_join() -> Path:
    src = ROOT / "tools" / "record_lines_host_join.cpp"
    if not HOST_JOIN.exists() or HOST_JOIN.stat().st_mtime < src.stat().st_mtime:
        HOST_JOIN.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", str(src), "-o", str(HOST_JOIN), "-lpthread"], check=True)
    return HOST_JOIN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["tiny", "small"], default="small")
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--build-only", action="store_true", help="build tools/_build/librecord_lines_host_join.so and leave")
    args = ap.parse_args()
    join = C.CDLL(str(build_host_join()))
    if args.build_only:
        return
    join.rl_host_join.restype = C.c_uint64
    join.rl_host_join.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_int]
    c = SHAPES[args.shape]
    nc, S = c["contigs"], args.samples
    index = [synthetic_panel(c["V"], PATHS, 20, seed=777 + i, multiallelic_frac=0.2) for i in range(nc)]
    pool = []
    for s in range(min(S, 16)):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    job = hmm.Job.cohort(index, [pool[s % len(pool)] for s in range(S)], hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5))
    rng = np.random.default_rng(20261020)
    plans = [random_plan(rng, ix) for ix in index]
    prefixes = []
    for k, p in enumerate(plans):   # about 60 bytes: CHROM .. FORMAT of a short variant
        rows = [("chr%d\t%d\t.\tA\tC\t.\tPASS\tAF=0.%03d;UK=%d;MA=0\tGT:GQ:GL:KC" % (k + 1, 1000 * r + 1, r % 1000, r % 300)).encode() for r in range(p.n_records)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.uint64)
        prefixes.append((off, np.frombuffer(b"".join(rows), np.uint8)))
    for _ in range(2):
        job.run()
    for k in range(nc):
        job.record_plan(k, plans[k])
        job.line_prefix(k, *prefixes[k])
    calls.form_record_text(job)
    lib, err = job._lib, C.create_string_buffer(1024)
    R = np.array([p.n_records for p in plans], np.uint64)
    n_lines = int(R.sum())
    rec_first = np.concatenate([[0], np.cumsum(np.tile(R, S))]).astype(np.uint64)
    poff = (C.c_void_p * nc)(*[p[0].ctypes.data for p in prefixes])
    pbytes = (C.c_void_p * nc)(*[p[1].ctypes.data for p in prefixes])
    prefix_bytes = sum(int(p[0][-1]) for p in prefixes)

    # the buffers of both routes are made once: a repeat times the calls, not numpy
    text_first = calls._record_text_first(job)
    n_text = int(text_first[-1])
    cap = calls.record_lines_bound(n_lines, S, prefix_bytes, n_text)
    off, text_arr = np.zeros(n_lines * S + 1, np.uint64), np.empty(max(n_text, 1), np.uint8)
    host_off, host_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    dev_off, dev_out = np.zeros(n_lines + 1, np.uint64), np.empty(max(cap, 1), np.uint8)
    line_first, byte_first = np.zeros(nc + 1, np.uint64), np.zeros(nc + 1, np.uint64)

    def check(rc):
        if rc:
            raise RuntimeError(err.value.decode(errors="replace"))

    T = {k: [] for k in ("a_fetch", "a_join_1", "a_join_16", "b_form", "b_fetch")}
    kernel_ms = []
    n_host = n_dev = 0
    for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
        t0 = time.perf_counter()
        check(lib.pg_job_fetch_record_text_packed(job.h, off.ctypes.data, text_arr.ctypes.data, n_text, err, 1024))
        t1 = time.perf_counter()
        joins = []
        for threads in (1, 16):
            ta = time.perf_counter()
            n_host = join.rl_host_join(nc, S, R.ctypes.data, rec_first.ctypes.data, off.ctypes.data, text_arr.ctypes.data, poff, pbytes, host_off.ctypes.data,
                                       host_out.ctypes.data, threads)
            joins.append(time.perf_counter() - ta)
        t2 = time.perf_counter()
        check(lib.pg_job_record_lines(job.h, err, 1024))
        t3 = time.perf_counter()
        check(lib.pg_job_record_lines_first(job.h, None, line_first.ctypes.data, byte_first.ctypes.data, err, 1024))
        n_dev = int(byte_first[-1])
        check(lib.pg_job_fetch_record_lines_packed(job.h, dev_off.ctypes.data, dev_out.ctypes.data, n_dev, err, 1024))
        t4 = time.perf_counter()
        if rep:
            for k, v in zip(T, (t1 - t0, joins[0], joins[1], t3 - t2, t4 - t3)):
                T[k].append(v)
            kernel_ms.append(job.record_lines_ms())
    host, dev = (host_off, host_out[:n_host]), (dev_off, dev_out[:n_dev])
    assert n_dev == n_host and np.array_equal(dev[1], host[1]), (n_dev, n_host)   # both routes: the same bytes
    assert np.array_equal(dev[0], host[0]) and int(line_first[-1]) == n_lines
    text_bytes, line_bytes = n_text, n_dev
    hosts = int((np.diff(dev[0].astype(np.int64)) == 0).sum())
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    # formula traffic of the three kernels: k_rlines_len reads 8 (S + 1) bytes of offsets a line and writes 4; k_rlines_emit reads them
    # again and the line's place (4), reads the texts and the prefixes of the lines it writes, writes the lines and 8 bytes a line
    traffic = n_lines * (2 * 8 * (S + 1) + 4 + 4 + 8) + 2 * line_bytes
    kms = float(np.median(kernel_ms))
    res = {"shape": args.shape, "samples": S, "contigs": nc, "lines": n_lines, "text_bytes": text_bytes, "prefix_bytes": prefix_bytes, "line_bytes": line_bytes,
           "lines_left_to_the_host": hosts, "repeats": args.repeats, "routes_agree": True}
    res.update({k: sp(v) for k, v in T.items()})
    res["pg_job_record_lines_kernels_ms"] = {"median": round(kms, 4), "min": round(min(kernel_ms), 4), "max": round(max(kernel_ms), 4)}
    res["kernels_formula_bytes"] = traffic
    res["kernels_GBps"] = round(traffic / kms / 1e6, 1) if kms > 0 else None
    res["kernels_fraction_of_hbm_peak"] = round(traffic / kms / 1e6 / HBM_PEAK_GBPS, 4) if kms > 0 else None
    med = lambda k: 1e3 * float(np.median(T[k]))
    res["route_a_ms"] = {"with_1_thread": round(med("a_fetch") + med("a_join_1"), 3), "with_16_threads": round(med("a_fetch") + med("a_join_16"), 3)}
    res["route_b_ms"] = {"total": round(med("b_form") + med("b_fetch"), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
