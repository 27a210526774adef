#!/usr/bin/env python3
"""The VCF lines of a SAMPLED cohort on the device: two routes from one job that has run and whose record text
is formed, on the shapes of tools/bench_sampled_record_fields.py (small: 512 chains as 64 samples x 8 contigs, 128 panel paths
sampled to 15 + the reference path).  Every chain is an index contig of its own; the fixed columns of the chains of a contig
differ in UK only.

  (a)  what the C ABI offered before: one pg_job_line_prefix per CHAIN with that chain's UK already in the bytes (the bytes are
       put together before the clock starts: the fetch of every chain's k-mer counts and the formatting are NOT in (a)'s time),
       pg_job_record_lines — the plain kernels of pg_record_lines.hip —, the packed fetch;
  (b)  one pg_job_line_prefix_strided per CONTIG with a slot per record, pg_job_record_lines — the slotted kernels of
       pg_record_lines.hip, which print every chain's UK at the slot —, the packed fetch.

One process, one warm-up, several repeats with their spread, the two routes alternating inside every repeat; each route starts
from a job without prefixes (the other route's are dropped off the clock, by attaching the plans anew).  Asserts that both
give the same bytes and offsets; prints medians with min and max: the prefix bytes uploaded, the upload, pg_job_record_lines (wall
and the kernels' _ms), the fetch, the totals.  Sets no threshold on time.

    python tools/bench_record_lines_slot.py --shape tiny|small|full [--repeats N]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_record_calls import random_plan  # noqa: E402
from bench_sampled_record_fields import PATHS, SHAPES, SIZE  # noqa: E402
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd import sampler as smp  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402


def fixed_columns(contig, plan, index):
    """per record (head, tail) of CHROM .. FORMAT around the digits of UK, as Graph::genotypes_fixed_columns prints them"""
    rec_var = np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))
    heads = [("chr%d\t%d\t.\tA\tC\t.\tPASS\tAF=0.25;UK=" % (contig + 1, int(index.variant_pos[v]) + 1)).encode() for v in rec_var]
    return rec_var, heads, b";MA=0\tGT:GQ:GL:KC"


def packed(strings):
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    return off, np.frombuffer(b"".join(strings), np.uint8)


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
    rng = np.random.default_rng(20261021)
    plans = [random_plan(rng, ix) for ix in index]
    for i in range(nc):
        job.record_plan_strided(i, nc, plans[i])
    job.run()
    job.record_text_packed()   # the text is formed before either route starts
    # the prefixes of both routes, before the clock starts
    columns = [fixed_columns(i, plans[i], index[i]) for i in range(nc)]
    slotted = []
    for rec_var, heads, tail in columns:
        off, data = packed([h + tail for h in heads])
        slotted.append((off, data, np.array([len(h) for h in heads], np.uint32)))
    per_chain = []
    for g in range(n):
        rec_var, heads, tail = columns[g % nc]
        uk = job.fetch(g).n_kmers[rec_var]
        per_chain.append(packed([h + str(int(u)).encode() + tail for h, u in zip(heads, uk)]))
    bytes_a = sum(int(p[0][-1]) + p[0].nbytes for p in per_chain)
    bytes_b = sum(int(p[0][-1]) + p[0].nbytes + p[2].nbytes for p in slotted)
    T = {k: [] for k in ("a_upload", "a_lines", "a_fetch", "a_total", "b_upload", "b_lines", "b_fetch", "b_total")}
    ms_a, ms_b = [], []
    got_a = got_b = None
    def fresh():
        """no prefix attached, the text formed: where a route starts (off the clock: a new plan drops the prefixes of the other
        route, so that neither route pays for freeing them)"""
        for i in range(nc):
            job.record_plan_strided(i, nc, plans[i])
        calls.form_record_text(job, False)

    for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
        fresh()
        t0 = time.perf_counter()
        for g in range(n):
            job.line_prefix(g, *per_chain[g])
        t1 = time.perf_counter()
        calls.form_record_lines(job)
        t2 = time.perf_counter()
        got_a = calls.fetch_record_lines_packed(job)
        t3 = time.perf_counter()
        ka = job.record_lines_ms()
        a = (t1 - t0, t2 - t1, t3 - t2, t3 - t0)
        fresh()
        t0 = time.perf_counter()
        for i in range(nc):
            job.line_prefix_strided(i, nc, slotted[i][0], slotted[i][1], slot=slotted[i][2])
        t1 = time.perf_counter()
        calls.form_record_lines(job)
        t2 = time.perf_counter()
        got_b = calls.fetch_record_lines_packed(job)
        t3 = time.perf_counter()
        kb = job.record_lines_ms()
        b = (t1 - t0, t2 - t1, t3 - t2, t3 - t0)
        assert got_a[1] == got_b[1] and np.array_equal(got_a[0], got_b[0]) and np.array_equal(got_a[2], got_b[2]) and np.array_equal(got_a[3], got_b[3])
        if rep:
            for k, v in zip(("a_upload", "a_lines", "a_fetch", "a_total"), a):
                T[k].append(v)
            for k, v in zip(("b_upload", "b_lines", "b_fetch", "b_total"), b):
                T[k].append(v)
            ms_a.append(ka); ms_b.append(kb)
    n_lines, n_bytes = len(got_b[0]) - 1, len(got_b[1])
    hosts = int((np.diff(got_b[0].astype(np.int64)) == 0).sum())
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    ms = lambda xs: {"median": round(float(np.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    out = {"shape": args.shape, "chains": n, "contigs": nc, "lines": n_lines, "lines_of_the_hosts": hosts, "line_bytes": n_bytes, "repeats": args.repeats,
           "routes_agree": True, "prefix_bytes_uploaded_a": bytes_a, "prefix_bytes_uploaded_b": bytes_b, "prefix_uploads_a": n, "prefix_uploads_b": nc}
    out.update({k: sp(v) for k, v in T.items()})
    out.update({"pg_job_record_lines_ms_a_plain_kernels": ms(ms_a), "pg_job_record_lines_ms_b_slot_kernels": ms(ms_b)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
