#!/usr/bin/env python3
"""The sample column per VCF record of a SAMPLED cohort: three routes from one job that has run to GT, GQ and
GL of every record of every chain, under the plan of tools/bench_record_calls.py (1-3 records per bubble, a tenth of the record
alleles undefined).  The protocol of tools/bench_record_gl.py: one process, one warm-up, several repeats with their spread.

  (a)  what genotype_cohort_sampled does today: the reduced panel and the bins of every chain back to the host, then per record
       normalise / fold / restrict to the defined alleles / likeliest genotype / quality / the four digits of log10, in long
       double on 16 host threads (vectorised numpy; a chain's groups depend on its own reduced panel and are part of the work);
  (b0) one pg_job_record_plan per chain, pg_job_record_calls + pg_job_record_gl, the per-chain fetches;
  (b)  one pg_job_record_plan_strided per contig, the same two calls, the two packed fetches.

For (b0) and (b) every repeat attaches the plans anew, forms records and values (the first call after a plan has changed makes
descriptors and lists and checks the ids), forms them again (the kernels alone) and fetches: set-up = attach + first - again.
Asserts that (b0) and (b) give the same bytes and that (a) agrees with them on every call and every GL value that is not
deferred; prints medians with min and max, the kernels' _ms and the bytes per record over PCIe.  Sets no threshold on time.

    python tools/bench_sampled_record_fields.py --shape tiny|small|full [--repeats N]
"""
import argparse
import ctypes as C
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_record_calls import THREADS, prepare, random_plan  # noqa: E402
from bench_record_gl import UNSURE, host_record_fields  # noqa: E402
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd import sampler as smp  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

SHAPES = {   # samples x contigs x bubbles; 128 panel paths sampled to 15 + the reference path
    "tiny": dict(samples=8, contigs=2, V=300),
    "small": dict(samples=64, contigs=8, V=2_000),      # 512 chains
    "full": dict(samples=512, contigs=8, V=2_000),      # 4096 chains
}
PATHS, SIZE = 128, 15


def form(job):
    err = C.create_string_buffer(1024)
    for f in (job._lib.pg_job_record_calls, job._lib.pg_job_record_gl):
        if f(job.h, err, 1024):
            raise RuntimeError(err.value.decode(errors="replace"))


def host_route(job, chain, plan, gl_off, res):
    batch = job.batches[chain]
    return host_record_fields(batch, plan, prepare(batch, plan), gl_off, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="small")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    c = SHAPES[args.shape]
    nc = c["contigs"]
    index = [synthetic_panel(c["V"], PATHS, 20, seed=777 + i, multiallelic_frac=0.2) for i in range(nc)]
    pool = []
    for s in range(min(c["samples"], 16)):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    samples = [pool[s % len(pool)] for s in range(c["samples"])]
    job, _, _ = smp.sample_cohort(index, samples, SIZE, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5),
                                  add_reference=True, want_paths=False)
    n = job.n_chains
    rng = np.random.default_rng(20261019)
    plans = [random_plan(rng, ix) for ix in index]   # over the ids of the whole panel: a reduced panel keeps the ids
    offsets = [calls.record_gl_offsets(p) for p in plans]
    n_rec = sum(plans[g % nc].n_records for g in range(n))
    n_val = sum(int(offsets[g % nc][-1]) for g in range(n))
    n_bins = sum(int(b.geno_off[-1]) for b in job.batches)
    panel_bytes = sum(b.kmer_off.nbytes + b.kmer_count.nbytes + b.allele_off.nbytes + b.allele_id.nbytes + b.allele_flags.nbytes +
                      b.allele_kmer_off.nbytes + b.allele_kmer_mask.nbytes + b.path_allele.nbytes for b in job.batches)
    for _ in range(2):
        job.run()
    bufs = job.fetch_all()
    T = {k: [] for k in ("a_total", "a_panels", "a_bins", "a_host", "b0_attach", "b0_first", "b0_again", "b0_fetch", "b_attach", "b_first", "b_again", "b_fetch")}
    ms_calls, ms_gl = [], []
    want = b0 = b = None
    with ThreadPoolExecutor(THREADS) as tp:
        for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
            t0 = time.perf_counter()
            job.batches = [job.fetch_panel(g) for g in range(n)]
            t1 = time.perf_counter()
            job.fetch_all(into=bufs)
            t2 = time.perf_counter()
            want = list(tp.map(lambda g: host_route(job, g, plans[g % nc], offsets[g % nc], bufs[g]), range(n)))
            t3 = time.perf_counter()
            a = (t3 - t0, t1 - t0, t2 - t1, t3 - t2)
            # (b0) a plan per chain
            t0 = time.perf_counter()
            for g in range(n):
                job.record_plan(g, plans[g % nc])
            t1 = time.perf_counter()
            form(job)
            t2 = time.perf_counter()
            form(job)
            t3 = time.perf_counter()
            b0 = (calls.fetch_record_calls_all(job), calls.fetch_record_gl_all(job))
            t4 = time.perf_counter()
            r0 = (t1 - t0, t2 - t1, t3 - t2, t4 - t3)
            # (b) a plan per contig, checked on the device, packed fetches
            t0 = time.perf_counter()
            for i in range(nc):
                job.record_plan_strided(i, nc, plans[i])
            t1 = time.perf_counter()
            form(job)
            t2 = time.perf_counter()
            form(job)
            t3 = time.perf_counter()
            b = (job.record_calls_packed(), job.record_gl_packed())
            t4 = time.perf_counter()
            r1 = (t1 - t0, t2 - t1, t3 - t2, t4 - t3)
            if rep:
                for k, v in zip(("a_total", "a_panels", "a_bins", "a_host"), a):
                    T[k].append(v)
                for k, v in zip(("b0_attach", "b0_first", "b0_again", "b0_fetch"), r0):
                    T[k].append(v)
                for k, v in zip(("b_attach", "b_first", "b_again", "b_fetch"), r1):
                    T[k].append(v)
                ms_calls.append(job.record_calls_ms()); ms_gl.append(job.record_gl_ms())
    (packed, first), (packed_gl, first_gl) = b
    deferred = unsure = finite = 0
    for g in range(n):
        g_calls, g_gl = packed[int(first[g]):int(first[g + 1])], packed_gl[int(first_gl[g]):int(first_gl[g + 1])]
        assert g_calls.tobytes() == b0[0][g].tobytes() and g_gl.tobytes() == b0[1][g].tobytes(), g   # (b0) and (b): the same bytes
        w_calls, w_gl = want[g]
        d = g_calls["flags"] == calls.PG_CALL_DEFERRED
        for f in ("allele_1", "allele_2", "gq"):
            assert np.array_equal(g_calls[f][~d], w_calls[f][~d]), (g, f)
        dg = (g_gl["mant"] == 0) & (g_gl["exp10"] == calls.PG_GL_DEFERRED)
        un = (w_gl["mant"] == 0) & (w_gl["exp10"] == UNSURE)
        deferred += int(dg.sum()); unsure += int(un.sum()); finite += int((g_gl["mant"] != 0).sum())
        cmp = ~dg & ~un
        assert np.array_equal(g_gl["mant"][cmp], w_gl["mant"][cmp]) and np.array_equal(g_gl["exp10"][cmp], w_gl["exp10"][cmp]), g
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    ms = lambda xs: {"median": round(float(np.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    setup = lambda p: [x + y - z for x, y, z in zip(T[p + "_attach"], T[p + "_first"], T[p + "_again"])]
    out = {"shape": args.shape, "chains": n, "panel_paths": PATHS, "sampled_paths": SIZE + 1, "records": n_rec, "gl_values": n_val, "finite": finite,
           "repeats": args.repeats, "gl_deferred": deferred, "host_unsure": unsure, "routes_agree": True}
    out.update({k: sp(v) for k, v in T.items()})
    out.update({"b0_setup": sp(setup("b0")), "b_setup": sp(setup("b")), "pg_job_record_calls_ms": ms(ms_calls), "pg_job_record_gl_ms": ms(ms_gl),
                "bytes_per_record_a": round((12.0 * n_bins + panel_bytes) / n_rec, 2), "bytes_per_record_b0": round((8.0 * n_rec + 4.0 * n_val) / n_rec, 2),
                "bytes_per_record_b": round((8.0 * n_rec + 4.0 * n_val) / n_rec, 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
