#!/usr/bin/env python3
"""The whole sample column per VCF record (GT, GQ and GL) from the device against the same formed on the host, at the shape and
under the plan of tools/bench_record_calls.py (its shape, plan and preparation are imported).  One process, one warm-up,
several repeats with their spread:

  (a) as a caller does it without pg_job_record_gl: pg_job_fetch_all of the bins, then per record normalise / fold / restrict
      to the defined alleles and renormalise / likeliest genotype / quality AND the four digits of log10 of every genotype's
      likelihood, in long double on 16 host threads (vectorised numpy, whole arrays at once);
  (b) pg_job_record_calls + pg_job_record_gl + both fetches.

Asserts that the two routes agree on every call and on every GL value the device did not defer; prints medians with min and
max, pg_job_record_gl_ms, and the bytes per record that cross PCIe on both routes.  Sets no threshold on time.

    python tools/bench_record_gl.py --shape small|full [--repeats N]
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
sys.path.insert(0, str(ROOT / "tools"))

import bench  # noqa: E402  (the shapes)
from bench_record_calls import THREADS, host_record_calls, prepare, random_plan  # noqa: E402
from pangenie_amd import calls, hmm  # noqa: E402
from pangenie_amd.panel import default_table_args, synthetic_panel, synthetic_sample_counts  # noqa: E402

LD = np.longdouble
UNSURE = -32766   # host only: the long double product lies within 1e-12 of a rounding boundary (not compared)


def digits(F):
    """(mant, exp10) of log10 of the likelihoods F (long double, any shape): four significant digits, rounded to nearest"""
    mant = np.zeros(F.shape, np.int16)
    exp = np.zeros(F.shape, np.int16)
    exp[F == 0] = calls.PG_GL_NEG_INF
    pos = (F > 0) & (F != 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log10(np.where(pos, F, LD(0.5)))
        a = np.abs(v)
        k = np.floor(np.log10(a)).astype(np.int64)
        s = a * np.power(LD(10), (3 - k).astype(LD))
        k = k - (s < 1000) + (s >= 10000)
        s = a * np.power(LD(10), (3 - k).astype(LD))
    fl = np.floor(s)
    r = (fl + (s - fl > LD(0.5))).astype(np.int64)
    k = np.where(r == 10000, k + 1, k)
    r = np.where(r == 10000, 1000, r)
    unsure = pos & (np.abs((s - fl) - LD(0.5)) < LD(1e-12))
    mant[pos] = np.where(v < 0, -r, r)[pos]
    exp[pos] = k[pos]
    mant[unsure] = 0
    exp[unsure] = UNSURE
    return mant, exp


def host_record_fields(batch, plan, groups, gl_off, res):
    """route (a): the calls as tools/bench_record_calls.py forms them, and the GL values of every record"""
    out = host_record_calls(batch, plan, groups, res)
    gl = np.zeros(int(gl_off[-1]), calls.GL_DTYPE)
    gl["exp10"] = calls.PG_GL_NEG_INF   # a key nothing folds onto
    if plan.n_records == 0:
        return out, gl
    aoff, goff = batch.allele_off.astype(np.int64), batch.geno_off.astype(np.int64)
    lik = np.ldexp(res.lik.astype(LD), res.lik_exp.astype(np.int64))
    for g in groups:
        A, var, sa, sb, kidx = g["A"], g["var"], g["sa"], g["sb"], g["kidx"]
        n, rows = len(var), np.arange(len(var))
        P = (res.allele_present[aoff[var][:, None] + np.arange(A)] != 0) & (res.kept[var][:, None] != 0)
        K = P[:, sa] & P[:, sb]
        L = np.where(K, lik[goff[var][:, None] + np.arange(len(sa))], LD(0))
        s = np.zeros(n, LD)
        for j in range(len(sa)):
            s = s + L[:, j]
        Q = np.where((s > 0)[:, None], L / np.where(s > 0, s, LD(1))[:, None], L)
        F = np.zeros(g["defined"].shape, LD)
        for j in range(len(sa)):
            F[rows, kidx[:, j]] = F[rows, kidx[:, j]] + np.where(K[:, j], Q[:, j], LD(0))
        F[~K.any(axis=1), 0] = LD(1)
        D = g["defined"]
        s2 = np.zeros(n, LD)
        for k in range(F.shape[1]):
            s2 = s2 + np.where(D[:, k], F[:, k], LD(0))
        renorm = g["undef"] & (s2 > 0)
        F = np.where(renorm[:, None], F / np.where(renorm, s2, LD(1))[:, None], F)
        mant, exp = digits(F)
        va, vb = g["gt1"], g["gt2"]
        at = gl_off[g["recs"]].astype(np.int64)[:, None] + vb * (vb + 1) // 2 + va
        gl["mant"][at[D]] = mant[D]
        gl["exp10"][at[D]] = exp[D]
    return out, gl


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
    rng = np.random.default_rng(20261019)
    plans = [random_plan(rng, ix) for ix in index]
    prepared = [prepare(ix, p) for ix, p in zip(index, plans)]
    offsets = [calls.record_gl_offsets(p) for p in plans]
    for i, p in enumerate(plans):   # once per index contig
        job.record_plan(i, p)
    nc = len(index)
    n_rec = sum(plans[i % nc].n_records for i in range(len(job.batches)))
    n_val = sum(int(offsets[i % nc][-1]) for i in range(len(job.batches)))
    n_bins = sum(int(b.geno_off[-1]) for b in job.batches)
    for _ in range(2):
        job.run()
    bufs = job.fetch_all()
    t_a, t_fetch, t_host, t_b, ms_gl, ms_calls = [], [], [], [], [], []
    want = got_calls = got_gl = None
    per_chain = lambda xs: [xs[i % nc] for i in range(len(job.batches))]
    with ThreadPoolExecutor(THREADS) as tp:
        for rep in range(args.repeats + 1):   # (the first repeat is the warm-up)
            t0 = time.perf_counter()
            job.fetch_all(into=bufs)
            t1 = time.perf_counter()
            want = list(tp.map(host_record_fields, job.batches, per_chain(plans), per_chain(prepared), per_chain(offsets), bufs))
            t2 = time.perf_counter()
            got_calls = job.record_calls()
            got_gl = job.record_gl()
            t3 = time.perf_counter()
            if rep:
                t_fetch.append(t1 - t0); t_host.append(t2 - t1); t_a.append(t2 - t0); t_b.append(t3 - t2)
                ms_gl.append(job.record_gl_ms()); ms_calls.append(job.record_calls_ms())
    deferred = unsure = finite = 0
    for (w_calls, w_gl), g_calls, g_gl in zip(want, got_calls, got_gl):
        d = g_calls["flags"] == calls.PG_CALL_DEFERRED
        for f in ("allele_1", "allele_2", "gq"):
            assert np.array_equal(g_calls[f][~d], w_calls[f][~d]), f
        dg = (g_gl["mant"] == 0) & (g_gl["exp10"] == calls.PG_GL_DEFERRED)
        un = (w_gl["mant"] == 0) & (w_gl["exp10"] == UNSURE)
        deferred += int(dg.sum()); unsure += int(un.sum()); finite += int((g_gl["mant"] != 0).sum())
        cmp = ~dg & ~un
        assert np.array_equal(g_gl["mant"][cmp], w_gl["mant"][cmp]) and np.array_equal(g_gl["exp10"][cmp], w_gl["exp10"][cmp])
    job.close()
    sp = lambda xs: {"median_ms": round(1e3 * float(np.median(xs)), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}
    ms = lambda xs: {"median": round(float(np.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    print(json.dumps({
        "shape": args.shape, "chains": len(job.batches), "records": n_rec, "gl_values": n_val, "finite": finite, "repeats": args.repeats,
        "gl_deferred": deferred, "host_unsure": unsure, "values_equal": True,
        "a_fetch_bins_then_host_fields": sp(t_a), "a_fetch_all": sp(t_fetch), "a_host_loop_16_threads": sp(t_host),
        "b_device_calls_gl_and_fetches": sp(t_b),
        "pg_job_record_gl_ms": ms(ms_gl), "pg_job_record_calls_ms": ms(ms_calls),
        "bytes_per_record_a": round(12.0 * n_bins / n_rec, 2), "bytes_per_record_b": round((8.0 * n_rec + 4.0 * n_val) / n_rec, 2),
    }))


if __name__ == "__main__":
    main()
