#!/usr/bin/env python3
"""Calls from the device against calls formed on the host, on the cohort_h16m shape of bench.py (the shape is imported;
bench.py is not touched).  One process, after a warm-up, several repeats with their spread:

  (a) the route of a caller who forms the calls on the host: pg_job_fetch_all of the bins, then normalise / likeliest
      genotype / genotype quality in long double on 16 host threads (vectorised numpy over the variants of one allele count
      at a time — the same operations in the same order as GenotypingResult, whole arrays at once);
  (b) pg_job_calls + pg_job_fetch_calls_all.

Prints the bytes that cross PCIe per variant on both routes, pg_job_calls_ms, and asserts that the two routes give the same
calls for every variant.  Sets no threshold on time.

    python tools/bench_calls.py --shape small|full [--repeats N]
"""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the shapes)
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

LD = np.longdouble
THREADS = 16


def host_calls(batch, res):
    """normalize / get_likeliest_genotype / get_genotype_quality (pangenie_amd/genotyping_result.py) for every variant of a
    chain at once: per allele count A, the keys of all such variants as columns, walked in the map's order."""
    V = batch.n_variants
    out = np.zeros(V, calls.CALL_DTYPE)
    out["allele_1"] = out["allele_2"] = 0xFFFF
    out["flags"] = calls.PG_CALL_NONE
    if V == 0:
        return out
    aoff = batch.allele_off.astype(np.int64)
    goff = batch.geno_off.astype(np.int64)
    A_of = np.diff(aoff)
    lik = np.ldexp(res.lik.astype(LD), res.lik_exp.astype(np.int64))
    for A in np.unique(A_of):
        A = int(A)
        idx = np.flatnonzero(A_of == A)
        sa, sb = np.triu_indices(A)   # bin order: (a, b), a <= b, lexicographic
        P = (res.allele_present[aoff[idx][:, None] + np.arange(A)] != 0) & (res.kept[idx][:, None] != 0)
        K = P[:, sa] & P[:, sb]
        L = np.where(K, lik[goff[idx][:, None] + np.arange(len(sa))], LD(0))
        s = np.zeros(len(idx), LD)
        for j in range(len(sa)):
            s = s + L[:, j]
        Q = np.where((s > 0)[:, None], L / np.where(s > 0, s, LD(1))[:, None], L)
        best = np.zeros(len(idx), LD)
        bj = np.zeros(len(idx), np.int64)
        for j in range(len(sa)):
            up = K[:, j] & (Q[:, j] >= best)
            best = np.where(up, Q[:, j], best)
            bj = np.where(up, j, bj)
        tie = np.zeros(len(idx), bool)
        for j in range(len(sa)):
            tie |= K[:, j] & (bj != j) & (np.abs(Q[:, j] - best) < 0.0000000001)
        ok = (best > 0) & ~tie
        pw = LD(1) - best
        with np.errstate(divide="ignore"):
            gq = np.where(pw > 0, (-10 * np.log10(np.where(pw > 0, pw, LD(1)))).astype(np.int64), 10000)
        ids = batch.allele_id
        sel = idx[ok]
        out["allele_1"][sel] = ids[aoff[sel] + sa[bj[ok]]]
        out["allele_2"][sel] = ids[aoff[sel] + sb[bj[ok]]]
        out["gq"][sel] = gq[ok]
        out["flags"][sel] = calls.PG_CALL_OK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["small", "full"], default="small")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    c = dict(bench.COHORTS_MORE["cohort_h16m"])
    if args.shape == "small":
        c.update(samples=64, V=2_000)   # 512 chains: still the kernels of the full shape
    index = [synthetic_panel(c["V"], c["H"], c["K"], seed=777 + i, multiallelic_frac=c["multi"]) for i in range(c["contigs"])]
    pool = []
    for s in range(min(c["samples"], c["distinct"])):
        kcs, covs = zip(*[synthetic_sample_counts(ix, seed=100_100 + 100 * s + i) for i, ix in enumerate(index)])
        pool.append((list(kcs), list(covs)))
    samples = [pool[s % len(pool)] for s in range(c["samples"])]
    job = hmm.Job.cohort(index, samples, hmm.ProbabilityTable(*default_table_args()), hmm.make_params(1.26, False, 1e-5))
    n_var = sum(b.n_variants for b in job.batches)
    n_bins = sum(int(b.geno_off[-1]) for b in job.batches)
    n_all = sum(int(b.allele_off[-1]) for b in job.batches)
    for _ in range(2):
        job.run()
    bufs = job.fetch_all()
    t_a, t_fetch, t_host, t_b, ms_k = [], [], [], [], []
    want = got = None
    with ThreadPoolExecutor(THREADS) as tp:
        for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
            t0 = time.perf_counter()
            job.fetch_all(into=bufs)
            t1 = time.perf_counter()
            want = list(tp.map(host_calls, job.batches, bufs))
            t2 = time.perf_counter()
            got = job.calls()
            t3 = time.perf_counter()
            if rep:
                t_fetch.append(t1 - t0); t_host.append(t2 - t1); t_a.append(t2 - t0); t_b.append(t3 - t2); ms_k.append(job.calls_ms())
    deferred = called = 0
    for w, g in zip(want, got):
        d = g["flags"] == calls.PG_CALL_DEFERRED
        deferred += int(d.sum())
        called += int((g["flags"] == calls.PG_CALL_OK).sum())
        no_call = np.isin(g["flags"], (calls.PG_CALL_NONE, calls.PG_CALL_NOT_UNIQUE))
        assert np.array_equal(no_call[~d], (w["flags"] == calls.PG_CALL_NONE)[~d])
        for f in ("allele_1", "allele_2", "gq"):
            assert np.array_equal(g[f][~d], w[f][~d]), f
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    print(json.dumps({
        "shape": args.shape, "chains": len(job.batches), "variants": n_var, "bins": n_bins, "repeats": args.repeats,
        "called": called, "deferred": deferred, "calls_equal": True,
        "a_fetch_bins_then_host_calls": sp(t_a), "a_fetch_all": sp(t_fetch), "a_host_loop_16_threads": sp(t_host),
        "b_device_calls_and_fetch": sp(t_b),
        "pg_job_calls_ms": {"median": round(float(np.median(ms_k)), 4), "min": round(min(ms_k), 4), "max": round(max(ms_k), 4)},
        "pcie_bytes_per_variant": {"a": round((12 * n_bins + n_var + n_all) / n_var, 2), "b": 8.0},
    }))


if __name__ == "__main__":
    main()
